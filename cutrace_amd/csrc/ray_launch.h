// ray_launch.h — the launch the three query kernels share (ray_query.hip, ray_shade.hip, ray_points.hip): one lane per ray or
// point, `lanes` lanes per workgroup, the launch record as the kernel's one argument.  Host code of a .hip file only.
#ifndef CUTRACE_AMD_RAY_LAUNCH_H
#define CUTRACE_AMD_RAY_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// `n` lanes of `kernel` over `L` with `lds` bytes of dynamic LDS per workgroup; returns a hipError_t as int
template <class Launch>
int launch_lanes(void (*kernel)(Launch), const Launch &L, uint32_t n, uint32_t lanes, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3((n + lanes - 1) / lanes), dim3(lanes), lds, stream, L);
  return (int)hipGetLastError();
}

#endif
