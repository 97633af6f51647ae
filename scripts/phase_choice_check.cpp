// phase_choice_check.cpp — phased_build (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space, composed the way a launch
// composes it (render_kernel.hip ctr_launch_phased): every build of both kernel lists x shape in {0, 1} x the switches
// CUTRACE_NO_OPAQUE_BUILD and CUTRACE_NO_PHASE_SPLIT.  One line per case:
//     <kv in hex> <shape> <no_opaque> <no_phase_split> <opq> <phased>
// Host only, no HIP; tests/test_phase_cpu.py states the rule.  Build:
//   g++ -std=c++17 -O2 -Icutrace_amd/csrc -Iinclude scripts/phase_choice_check.cpp cutrace_amd/csrc/kernel_choice.cpp
#include <cstdio>

#include "kernel_choice.h"

int main() {
  static const uint32_t builds[] = {
#define X(kv) (kv),
      CTR_RENDER_KERNELS(X) CTR_LENS_KERNELS(X)
#undef X
  };
  for (uint32_t kv : builds)
    for (uint32_t shape = 0; shape < 2; shape++)
      for (int no_opq = 0; no_opq < 2; no_opq++)
        for (int no_split = 0; no_split < 2; no_split++) {
          const uint32_t opq = opaque_build(kv, shape, no_opq != 0);
          printf("%04x %u %d %d %u %d\n", (unsigned)kv, (unsigned)shape, no_opq, no_split, (unsigned)opq, (int)phased_build(opq, no_split != 0));
        }
  // the function itself on values no launch hands it
  for (uint32_t opq = 0; opq < 4; opq++)
    for (int no_split = 0; no_split < 2; no_split++) printf("raw %u %d %d\n", (unsigned)opq, no_split, (int)phased_build(opq, no_split != 0));
  return 0;
}
