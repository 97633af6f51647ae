// vec3.h — the reference's inc/vector.hpp on three floats, same operation order: every kernel of the library (the render kernel,
// the ray queries' walk and shading) forms its geometry with these, which is what makes their results the same bits.
// Device code only: include it from a .hip translation unit, after hip_runtime.h.  Unnamed namespace, one copy per
// translation unit.
#ifndef CUTRACE_AMD_VEC3_H
#define CUTRACE_AMD_VEC3_H

#include <math.h>

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 vscale(V3 a, float f) { return mk(f * a.x, f * a.y, f * a.z); }
__device__ __forceinline__ V3 vmul(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ float vdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 vcross(V3 a, V3 o) {
  return mk(a.y * o.z - a.z * o.y, a.z * o.x - a.x * o.z, a.x * o.y - a.y * o.x);
}
__device__ __forceinline__ float vnorm(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ V3 vnormalized(V3 a) { return vscale(a, 1.0f / vnorm(a)); }
// matrix::determinant, vector.hpp:218-224 (columns c0,c1,c2)
__device__ __forceinline__ float det3(V3 c0, V3 c1, V3 c2) {
  float a = c0.x, b = c1.x, c = c2.x, d = c0.y, e = c1.y, f = c2.y, g = c0.z, h = c1.z, i = c2.z;
  return a * e * i + b * f * g + c * d * h - c * e * g - a * f * h - b * d * i;
}
// std::min / std::max as the host-compiled reference binds the unqualified calls
__device__ __forceinline__ float smin(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }

}  // namespace

#endif
