// shape_choice_check.cpp — launch_shape (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space, one line per case:
// every build of CTR_RENDER_KERNELS and CTR_LENS_KERNELS x n_oloop in {0, 1} x head_mesh in {0, 1}, as
//   <kv in hex> <n_oloop> <head_mesh> <shape>
// then "shapes" and the KVs of CTR_SHAPE_KERNELS.  tests/test_shape_choice_cpu.py states what the answers must be.
//
//   g++ -std=c++17 -Iinclude -Icutrace_amd/csrc scripts/shape_choice_check.cpp cutrace_amd/csrc/kernel_choice.cpp
#include <cstdio>

#include "cutrace_amd.h"
#include "kernel_choice.h"

int main() {
  static const uint32_t builds[] = {
#define X(kv) (kv),
      CTR_RENDER_KERNELS(X) CTR_LENS_KERNELS(X)
#undef X
  };
  for (uint32_t kv : builds)
    for (uint32_t n_oloop = 0; n_oloop < 2; n_oloop++)
      for (int head_mesh = 0; head_mesh < 2; head_mesh++)
        printf("%04x %u %d %u\n", (unsigned)kv, (unsigned)n_oloop, head_mesh, (unsigned)launch_shape(kv, n_oloop, head_mesh != 0));
  printf("shapes\n");
#define X(kv) printf("%04x\n", (unsigned)(kv));
  CTR_SHAPE_KERNELS(X)
#undef X
  return 0;
}
