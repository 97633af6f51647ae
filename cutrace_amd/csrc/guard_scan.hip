// guard_scan.hip — the device half of the guard's plane scan (guard_scan.h; the host half is guard.cpp): one bit per triangle
// plane, set when a probe lies in the plane.
//
// One kernel of mesh_update.hip's shape: a lane owns what it writes, reads only what an earlier launch or copy on the same
// stream wrote, and ends.  No LDS, no atomics, no waiting between workgroups: nothing here can spin.
//   One lane per plane of the flat array (56 bytes, seven 8-byte loads).  The probe loop's index is the same in every lane of
//   a wave, so a probe record is a scalar load.  __ballot collects the wave's 64
//   answers, the wave's first lane writes them as one 8-byte vector store.  Lanes past the end vote 0; a wave that lies past
//   the end entirely writes nothing.
//
// Numerics: guard_scan.h is f64 +, -, *, |x|, max and compares alone; the library's -ffp-contract=off (build.py HIP_FLAGS) and
// the pragma below keep every one of them the single correctly rounded operation the host performs.
//
// Memory: 56 bytes in, one bit out per plane; 64 000 planes are 3.6 MB, a microsecond of HBM time.  The call is bound by the
// launch and the wait for the words, not by the kernel.
#include <hip/hip_runtime.h>

#include "guard_scan.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t GS_THREADS = 256;
static_assert(GS_THREADS % 64 == 0, "a wave writes one word");

__global__ void __launch_bounds__(GS_THREADS) guard_scan_kernel(const double *__restrict__ planes, uint32_t n,
                                                                const GuardProbe *__restrict__ probes, uint32_t n_points, uint32_t n_probes,
                                                                unsigned long long *__restrict__ words) {
  const uint32_t k = blockIdx.x * GS_THREADS + threadIdx.x;
  bool risky = false;
  if (k < n) {
    double q[CTR_PLANE_DOUBLES];
    const double *src = planes + (size_t)CTR_PLANE_DOUBLES * k;
    for (int j = 0; j < CTR_PLANE_DOUBLES; j++) q[j] = src[j];
    risky = plane_is_risky(q, probes, n_points, n_probes);
  }
  const unsigned long long mask = __ballot(risky);  // wave64: one bit per lane, lane 0 at bit 0
  if ((threadIdx.x & 63u) == 0u && k < n) words[k >> 6] = mask;
}

}  // namespace

int ctr_launch_guard_scan(const double *planes, uint32_t n, const GuardProbe *probes, uint32_t n_points, uint32_t n_probes, uint64_t *words,
                          void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(guard_scan_kernel, dim3((n + GS_THREADS - 1) / GS_THREADS), dim3(GS_THREADS), 0, (hipStream_t)stream, planes, n, probes,
                     n_points, n_probes, (unsigned long long *)words);
  return (int)hipGetLastError();
}
