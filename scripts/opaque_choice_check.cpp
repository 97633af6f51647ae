// opaque_choice_check.cpp — opaque_build (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space, and the lemma it rests
// on checked against the host code that decides it.  Three sections:
//   every build of CTR_RENDER_KERNELS and CTR_LENS_KERNELS x shape in {0, 1} x switch in {0, 1}, one line per case:
//     <kv in hex> <shape> <no_opaque> <opq>
//   "lds": per build of CTR_SHAPE_KERNELS x bounces 0..15 x (any_bounce, need_cold) in {(0,0), (1,0), (1,1)}:
//     <kv in hex> <bounces> <any_bounce> <need_cold> <LDS bytes per wave of the launch: lds_bytes_per_wave, which takes no opaque build>
//   "materials": one material whose transparency is each of a list of floats, through material_records (what flatten_scene and
//   ctr_scene_set_materials run) and then choose_kernel over every user mask and entry:
//     <transparency bits in hex> <all_opaque> <number of choices with KV_ANYHIT>
// tests/test_opaque_choice_cpu.py states what the answers must be.
//
//   g++ -std=c++17 -Iinclude -Icutrace_amd/csrc scripts/opaque_choice_check.cpp cutrace_amd/csrc/{kernel_choice,scene_flatten,guard,bvh}.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "cutrace_amd.h"
#include "kernel_choice.h"
#include "scene_flatten.h"

int main() {
  static const uint32_t builds[] = {
#define X(kv) (kv),
      CTR_RENDER_KERNELS(X) CTR_LENS_KERNELS(X)
#undef X
  };
  static const uint32_t shaped[] = {
#define X(kv) (kv),
      CTR_SHAPE_KERNELS(X)
#undef X
  };
  for (uint32_t kv : builds)
    for (uint32_t shape = 0; shape < 2; shape++)
      for (int off = 0; off < 2; off++) printf("%04x %u %d %u\n", (unsigned)kv, (unsigned)shape, off, (unsigned)opaque_build(kv, shape, off != 0));
  printf("lds\n");
  for (uint32_t kv : shaped)
    for (int bounces = 0; bounces <= 15; bounces++)
      for (int k = 0; k < 3; k++) {
        const bool any_bounce = k > 0, need_cold = k > 1;
        const StackShape st = stack_shape(bounces, any_bounce, need_cold);
        printf("%04x %d %d %d %zu\n", (unsigned)kv, bounces, (int)any_bounce, (int)need_cold, lds_bytes_per_wave(kv, st));
      }
  printf("materials\n");
  const float ts[] = {0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), 1e-30f, 9.9e-7f, 1e-6f,
                      0.25f, 1.0f, -0.25f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  for (float t : ts) {
    FlatScene F;
    ctr_material m[2];
    memset(m, 0, sizeof(m));
    m[0].type = m[1].type = CTR_MAT_PHONG;
    m[0].reflexivity = 0.3f;
    m[1].transparency = t;  // (the second of two: every record counts, not the first alone)
    material_records(F, m, 2);
    unsigned n_anyhit = 0;
    for (uint32_t user = 0; user < 16384u; user++)  // every CTR_VAR_* bit there is
      for (int entry = KE_HOST; entry <= KE_DEVICE_LENS_SS; entry++)
        for (int flags = 0; flags < 8; flags++) {
          const KernelFacts f = {user, F.all_opaque, (flags & 1) != 0, (flags & 2) != 0, (KernelEntry)entry, (flags & 4) != 0,
                                 stack_shape(5, F.any_bounce, F.need_cold), F.fast_pow_ok};
          const KernelChoice c = choose_kernel(f);
          if (c.reject == KR_NONE && (c.kv & KV_ANYHIT)) n_anyhit++;
        }
    uint32_t bits;
    memcpy(&bits, &t, sizeof(bits));
    printf("%08x %d %u\n", (unsigned)bits, (int)F.all_opaque, n_anyhit);
  }
  return 0;
}
