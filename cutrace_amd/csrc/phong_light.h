// phong_light.h — the per-light arithmetic of phong (inc/shading.hpp:64-99) for the per-lane kernels: the radiance queries
// (ray_shade.hip) and the surface shading queries (ray_points.hip) form it with these two functions, so the two cannot
// drift apart.  (The render kernel keeps its own wave-wide form, render_kernel.hip "phong".)
// Device code only: include it from a .hip translation unit, after hip_runtime.h.  Unnamed namespace, one copy per
// translation unit.
#ifndef CUTRACE_AMD_PHONG_LIGHT_H
#define CUTRACE_AMD_PHONG_LIGHT_H

#include <math.h>

#include "cutrace_amd.h"
#include "scene_device.h"
#include "vec3.h"

namespace {

// shading.hpp:79-85: direction and distance to a light as `sun` and `point_light` give them, and the shadow ray
// {*hit, direction.normalized()} with max_dist = distance * |direction| (shading.hpp:80)
struct LightRay {
  V3 dir;      // direction.normalized()
  float dist;  // distance * direction.norm()
};
__device__ __forceinline__ LightRay light_ray(const DLight Lg, V3 hit) {
  const V3 lg_v = mk(Lg.vx, Lg.vy, Lg.vz);
  V3 direction;
  float distance;
  if (Lg.type == CTR_LIGHT_SUN) {  // default_schema.hpp:280-283
    direction = vscale(lg_v, -1.0f);
    distance = INFINITY;
  } else {                         // default_schema.hpp:305-308
    const V3 diff = vsub(lg_v, hit);
    distance = vnorm(diff);
    direction = vscale(diff, 1.0f / distance);
  }
  const float dir_norm = vnorm(direction);
  LightRay R;
  R.dir = vscale(direction, 1.0f / dir_norm);
  R.dist = distance * dir_norm;
  return R;
}

// shading.hpp:86-95: what a light whose shadow factor came out below 1 adds to phong's `final`.  nn: normal.normalized(),
// in_dn: incoming->dir.normalized(), nd: the shadow ray's direction (it IS direction.normalized()).
// EXACT: IEEE half vector and f64 pow rounded once (CTR_VAR_EXACT_POW); else the render's fast specular term: 1-ulp
// v_rsq_f32 for the half vector, exp2(e * log2(x)) on the transcendental pipe, phong_exp == 0 -> 1.
template <bool EXACT>
__device__ __forceinline__ V3 lit_term(const DMat M, const DLight Lg, V3 nn, V3 in_dn, V3 nd, float shadow_fac) {
  const V3 diffuse = mk(M.cx, M.cy, M.cz);
  const V3 specular = vscale(diffuse, M.specular);  // default_schema.hpp:328
  const V3 color = mk(Lg.cx, Lg.cy, Lg.cz);
  const float fd_ = smax(0.0f, vdot(nn, nd));
  const V3 ld = vmul(diffuse, color);
  const V3 hsum = vadd(vscale(in_dn, -1.0f), nd);
  const V3 hv = EXACT ? vnormalized(hsum) : vscale(hsum, __builtin_amdgcn_rsqf(vdot(hsum, hsum)));
  const float sx = smax(0.0f, vdot(nn, hv));
  float fs;
  if (EXACT) fs = (float)pow((double)sx, (double)M.phong_exp);  // f64, rounded once
  else fs = (M.phong_exp == 0.0f) ? 1.0f : __builtin_amdgcn_exp2f(M.phong_exp * __builtin_amdgcn_logf(sx));
  const V3 ls = vmul(specular, color);
  return vscale(vadd(vscale(ld, fd_), vscale(ls, fs)), 1 - shadow_fac);
}

}  // namespace

#endif
