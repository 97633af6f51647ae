// frame_images.hip — the display quantiser of include/cutrace_images.h: float depth / colour / normal planes to the bytes of the
// host's ctr_quantise_depth / _color / _normal (host/images.cpp:181-209, the reference's inc/images.hpp:27-29,48-54,73-76).
//
// Numerics.  Byte equality with the host needs every float operation rounded once, in the host's order.  The file is
// compiled with the library's -ffp-contract=off, but it does not rely on that.  The pragma below switches contraction off
// for -ffp-contract=on, fast-honor-pragmas and the compiler's default; -ffp-contract=fast disregards pragmas, so every
// product that feeds a sum also passes through rounded(), an empty asm statement the backend cannot look through: by the
// time the sum is formed the product is a rounded value in a register, and there is nothing left to fuse.  Checked on the
// gfx950 assembly under all five modes: the same instructions, and the only fused multiply-adds are those of the division
// and square-root expansions.  Division and square root are the IEEE ones of -fhip-fp32-correctly-rounded-divide-sqrt
// (build.py HIP_FLAGS); that flag the file does rely on.
//
// Memory.  28 bytes are read and 9 written per pixel, nothing is reused: the kernel is bound by memory.  One lane takes one
// pixel of every plane: dword and dwordx3 loads that a wave covers contiguously, byte stores that a wave covers contiguously.
// Inputs need 4-byte alignment only, outputs none, every n works without a head or a tail.  A widened kernel — four pixels
// per lane, dwordx4 / dwordx3 loads, the 12 output bytes of a group as one aligned dwordx3 store, byte-wise head and tail per
// plane — was built and measured against this one on the 1080p frame: 0.015 ms against this kernel's 0.014 ms
// (profiles/images/widened_ab.txt).  It bought nothing and was dropped.
#include <hip/hip_runtime.h>

#include "frame_images.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t FI_THREADS = 256;
constexpr uint64_t FI_MAX_BLOCKS = 1u << 20;  // beyond that the lanes stride over the frame

// v, rounded and in a register: a product that went through here cannot be contracted into the sum that uses it
// (no instruction is emitted)
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the conversion the host leaves undefined outside [0, 256): clamped to [0, 255] (NaN fails the first test: 0), truncated
__device__ __forceinline__ uint32_t to_byte(float v) {
  const float lo = (v > 0.0f) ? v : 0.0f;
  const float c = (lo < 255.0f) ? lo : 255.0f;
  return (uint32_t)(int)c;
}

__device__ __forceinline__ uint32_t depth_byte(float v, float max_d) {
  if (!__builtin_isfinite(v)) return 0u;
  const float t = max_d - v;
  const float p = 255.0f * t;
  const float q = p / max_d;
  return to_byte(q);
}

__device__ __forceinline__ uint32_t color_byte(float v) {
  const float lo = (0.0f < v) ? v : 0.0f;   // std::max(0.0f, v)
  const float c = (lo < 1.0f) ? lo : 1.0f;  // std::min(1.0f, lo)
  const float p = 255.0f * c;
  return to_byte(p);
}

__device__ __forceinline__ uint32_t normal_component(float f, float c) {
  const float a = f * c;
  const float h = rounded(0.5f * a);
  const float m = 0.5f + h;
  const float p = 255.0f * m;
  return to_byte(p);
}

__device__ __forceinline__ void normal_bytes(float x, float y, float z, uint32_t *b) {
  const float xx = rounded(x * x);
  const float yy = rounded(y * y);
  const float zz = rounded(z * z);
  const float sxy = xx + yy;
  const float s = sxy + zz;
  const float len = __builtin_sqrtf(s);
  if ((double)len <= 1e-6) {
    b[0] = b[1] = b[2] = 0u;
    return;
  }
  const float f = 1.0f / len;
  b[0] = normal_component(f, x);
  b[1] = normal_component(f, y);
  b[2] = normal_component(f, z);
}

enum Plane { DEPTH, COLOR, NORMAL };

// the three bytes of pixel i of a plane
template <Plane P>
__device__ __forceinline__ void pixel_bytes(const float *in, uint64_t i, float max_d, uint32_t *b) {
  if (P == DEPTH) {
    b[0] = b[1] = b[2] = depth_byte(in[i], max_d);
  } else if (P == COLOR) {
    for (int k = 0; k < 3; k++) b[k] = color_byte(in[3 * i + k]);
  } else {
    normal_bytes(in[3 * i], in[3 * i + 1], in[3 * i + 2], b);
  }
}

// pixel i of one plane
template <Plane P>
__device__ __forceinline__ void plane_pixel(const float *in, uint8_t *out, uint64_t i, float max_d) {
  uint32_t b[3];
  pixel_bytes<P>(in, i, max_d, b);
  out[3 * i] = (uint8_t)b[0];
  out[3 * i + 1] = (uint8_t)b[1];
  out[3 * i + 2] = (uint8_t)b[2];
}

__global__ void __launch_bounds__(FI_THREADS) frame_images_kernel(const ImagesLaunch L) {
  float max_d = L.max_depth;
  if (L.counters) max_d = __uint_as_float((uint32_t)L.counters[1]);
  const uint64_t stride = (uint64_t)gridDim.x * FI_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * FI_THREADS + threadIdx.x; i < L.n; i += stride) {
    if (L.depth8) plane_pixel<DEPTH>(L.depth, L.depth8, i, max_d);
    if (L.color8) plane_pixel<COLOR>(L.color, L.color8, i, 0.0f);
    if (L.normal8) plane_pixel<NORMAL>(L.normal, L.normal8, i, 0.0f);
  }
}

}  // namespace

int ctr_launch_images(const ImagesLaunch &L, void *stream) {
  if (L.n == 0) return 0;
  const uint64_t blocks = (L.n + FI_THREADS - 1) / FI_THREADS;
  const dim3 grid((uint32_t)(blocks < FI_MAX_BLOCKS ? blocks : FI_MAX_BLOCKS));
  hipLaunchKernelGGL(frame_images_kernel, grid, dim3(FI_THREADS), 0, (hipStream_t)stream, L);
  return (int)hipGetLastError();
}
