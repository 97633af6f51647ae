// kernel_choice_check.cpp — choose_kernel (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space, one answer per line
// in a fixed order: tests/test_kernel_choice.py compares them with tests/golden/kernel_choice.npz, recorded from the
// launch path as it was before there was a chooser (tests/golden/kernel_choice.md).
//
//   g++ -std=c++17 -Iinclude -Icutrace_amd/csrc scripts/kernel_choice_check.cpp cutrace_amd/csrc/kernel_choice.cpp
//
// Order, outermost first: 6 entries (KernelEntry) x 512 user masks (bit k of the index = MASK_BITS[k]) x 8 scene-flag triples
// (bit 0 all_opaque, bit 1 big mesh, bit 2 merged tree usable) x deliverable (no, yes) x 4 stack shapes (SHAPES).
// A line is the build's KV in hex, or 0xf000 + KernelReject for a combination without a build.  After the cases: "list"
// and the KVs of CTR_RENDER_KERNELS; then "neutral" and how many of the sampled cases CTR_VAR_NO_REORDER and
// CTR_VAR_IMAGE_ORDER_FIRST changed (must be 0); then "slowpow" and how many cases, with fast_pow_ok false (every case above
// has it true), get another answer than the same case with CTR_VAR_EXACT_POW among the caller's bits (must be 0).
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
  // what the other outputs say must be what the KV says
  if (c.direct != ((c.kv & KV_HOSTOUT) != 0) || c.merged != ((c.kv & KV_MERGE) != 0)) return 0xffffu;
  return c.kv;
}

int main() {
  unsigned n = 0, moved = 0, slowpow = 0;
  for (int entry = 0; entry < 6; entry++)
    for (unsigned m = 0; m < 512; m++) {
      uint32_t user = 0;
      for (int k = 0; k < 9; k++)
        if (m >> k & 1) user |= MASK_BITS[k];
      for (unsigned flags = 0; flags < 8; flags++)
        for (int deliverable = 0; deliverable < 2; deliverable++)
          for (const StackShape &st : SHAPES) {
            KernelFacts f{user, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (KernelEntry)entry, deliverable != 0, st};
            const unsigned a = answer(f);
            printf("%04x\n", a);
            {  // a scene outside the fast specular path's domain: the launch CTR_VAR_EXACT_POW would get
              KernelFacts slow = f, exact = f;
              slow.fast_pow_ok = false;
              exact.user = user | CTR_VAR_EXACT_POW;
              slowpow += answer(slow) != answer(exact);
            }
            if (n++ % 7 == 0)  // a sample: the bits that order the tiles choose no build
              for (uint32_t extra : {CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST, CTR_VAR_NO_REORDER | CTR_VAR_IMAGE_ORDER_FIRST}) {
                f.user = user | extra;
                moved += answer(f) != a;
              }
          }
    }
  printf("list\n");
#define X(kv) printf("%04x\n", (unsigned)(kv));
  CTR_RENDER_KERNELS(X)
#undef X
  printf("neutral\n%u\n", moved);
  printf("slowpow\n%u\n", slowpow);
  return 0;
}
