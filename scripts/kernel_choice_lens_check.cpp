// kernel_choice_lens_check.cpp — choose_kernel (cutrace_amd/csrc/kernel_choice.cpp) for the two lens entries over their whole
// input space, one answer per line in a fixed order, for tests/test_lens_cpu.py.  scripts/kernel_choice_check.cpp does the same
// for the six entries that were there before and keeps its output.
//
//   g++ -std=c++17 -Iinclude -Icutrace_amd/csrc scripts/kernel_choice_lens_check.cpp cutrace_amd/csrc/kernel_choice.cpp
//
// Order, outermost first: 2 entries (KE_DEVICE_LENS, KE_DEVICE_LENS_SS) x 512 user masks (bit k of the index = MASK_BITS[k])
// x 8 scene-flag triples (bit 0 all_opaque, bit 1 big mesh, bit 2 merged tree usable) x deliverable (no, yes) x 4 stack shapes.
// A line is the build's KV in hex, or 0xf000 + KernelReject, or 0xffff when the chooser's outputs contradict each other.  After
// the cases: "list" and the KVs of CTR_LENS_KERNELS; "render" and how many KVs CTR_RENDER_KERNELS has; "reject" and KR_LENS's line; "neutral" and how many
// cases CTR_VAR_NO_REORDER and CTR_VAR_IMAGE_ORDER_FIRST changed (every case is tried; must be 0).
#include <cstdio>
#include <initializer_list>

#include "cutrace_amd.h"
#include "kernel_choice.h"

static const uint32_t MASK_BITS[9] = {CTR_VAR_NO_PREFILTER, CTR_VAR_NO_ANYHIT, CTR_VAR_NO_CLUSTER, CTR_VAR_STATS, CTR_VAR_EXACT_POW,
                                      CTR_VAR_NO_OCC6, CTR_VAR_NO_DIRECT, CTR_VAR_MERGE, CTR_VAR_IGNORE_TRANSPARENT};
// the first and third fit the 6-wave build, the second and fourth are the smallest that do not
static const StackShape SHAPES[4] = {{5, 4}, {6, 4}, {2, 10}, {3, 10}};

static unsigned answer(const KernelFacts &f) {
  const KernelChoice c = choose_kernel(f);
  if (c.reject != KR_NONE) return 0xf000u + (unsigned)c.reject;
  if (c.direct || c.merged || (c.kv & (KV_HOSTOUT | KV_MERGE))) return 0xffffu;  // a lens launch is neither
  return c.kv;
}

int main() {
  unsigned moved = 0;
  for (KernelEntry entry : {KE_DEVICE_LENS, KE_DEVICE_LENS_SS})
    for (unsigned m = 0; m < 512; m++) {
      uint32_t user = 0;
      for (int k = 0; k < 9; k++)
        if (m >> k & 1) user |= MASK_BITS[k];
      for (unsigned flags = 0; flags < 8; flags++)
        for (int deliverable = 0; deliverable < 2; deliverable++)
          for (const StackShape &st : SHAPES) {
            KernelFacts f{user, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, entry, deliverable != 0, st};
            const unsigned a = answer(f);
            printf("%04x\n", a);
            for (uint32_t extra : {CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST, CTR_VAR_NO_REORDER | CTR_VAR_IMAGE_ORDER_FIRST}) {
              f.user = user | extra;
              moved += answer(f) != a;
            }
          }
    }
  printf("list\n");
#define X(kv) printf("%04x\n", (unsigned)(kv));
  CTR_LENS_KERNELS(X)
#undef X
  unsigned n_render = 0;
#define X(kv) n_render++;
  CTR_RENDER_KERNELS(X)
#undef X
  printf("render\n%u\nreject\n%04x\nneutral\n%u\n", n_render, 0xf000u + (unsigned)KR_LENS, moved);
  return 0;
}
