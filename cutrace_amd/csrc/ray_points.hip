// ray_points.hip — the kernel behind ctr_shade_points (include/cutrace_rays.h): phong at points from memory.
//
// What it restates (reference, file:line), operation for operation, with the numerics of ray_shade.hip
// (-ffp-contract=off, IEEE division and square root):
//   phong               inc/shading.hpp:64-99       ambient + per light: shadow ray, diffuse and specular terms
//   shadow_intensity    inc/shading.hpp:22-45       a loop of nearest casts from (float)((double)last_hit + 1e-3)
// on top of the per-lane walk of ray_walk.h; the per-light arithmetic is phong_light.h's, shared with ray_shade.hip.
//
// ONE LANE = ONE POINT.  There is no cast in front and no recursion behind, so nothing lets the lanes of a wave drift
// apart over the lights as ray_shade.hip's do: the light loop is wave-uniform (the DLight record and the count sit in
// SGPRs), and per light there is ONE inner loop of casts through ONE call site, which the wave leaves when none of its
// lanes is inside its shadow loop any more.  Every lane's shadow ray of a trip runs towards the same light; a lane whose
// loop ended earlier sits the remaining trips out (masked), its shadow factor kept.  The colour accumulates in
// registers.  The only LDS is the walk's stack ([entry][lane], none under CTR_POINTS_LINEAR); no scratch memory.
//
// A lane whose point, normal or view direction is degenerate computes what the reference's arithmetic gives (NaNs
// where it gives NaNs); a NaN shadow ray is a miss of `cast`, and a NaN distance fails `t < max_dist`: its loop ends at
// the first trip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "cutrace_rays.h"
#include "phong_light.h"
#include "ray_launch.h"
#include "ray_points.h"
#include "ray_walk.h"

namespace {

constexpr int RP_THREADS = CTR_POINTS_THREADS;
enum : uint32_t { RP_LINEAR = 1u, RP_EXACT = 2u };

// The lights are read through the constant address space: the index is wave-uniform and no launch writes the array, so
// a record is one scalar load into SGPRs (through the generic pointer the kernel's own stores would make it a vector
// load per lane).
#define CADDR __attribute__((address_space(4)))
__device__ __forceinline__ DLight load_light(const CADDR DLight &G) {
  DLight r;
  r.type = G.type;
  r.vx = G.vx; r.vy = G.vy; r.vz = G.vz;
  r.cx = G.cx; r.cy = G.cy; r.cz = G.cz;
  r.pad = 0.0f;
  return r;
}

template <uint32_t K>
__global__ __launch_bounds__(RP_THREADS) void ray_points_kernel(PointsLaunch L) {
  constexpr uint32_t V = (K & RP_LINEAR) ? RQ_LINEAR : 0u;
  constexpr bool EXACT = (K & RP_EXACT) != 0;
  extern __shared__ uint32_t rp_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RP_THREADS + threadIdx.x;
  if (i >= L.n_points) return;
  const Scene S = make_scene(L.scene, 0u);  // every cast of phong's shadow_intensity passes ignore_transparent = false
  uint32_t *const stk = rp_stack + threadIdx.x;
  const DMat *const mats = L.scene.mats;
  const CADDR DLight *const lights = (const CADDR DLight *)L.lights;
  const uint32_t n_light = L.n_light;
  const bool opaque = L.all_opaque != 0u;
  const bool want_color = L.color != nullptr;

  const size_t i3 = (size_t)i * 3;
  const V3 hit = mk(L.point[i3], L.point[i3 + 1], L.point[i3 + 2]);  // phong's *hit
  // the material: the one named, or the named object's; `miss` is ray_color's answer for no hit (shading.hpp:119),
  // `bad` an index that names nothing (nothing is read for it)
  bool miss = false, bad = false;
  DMat M{};
  V3 nn = mk(0, 0, 0), in_dn = mk(0, 0, 0), fin = mk(0, 0, 0);
  if (want_color) {
    int32_t m = L.material;
    if (L.obj_arr) {
      const int32_t o = L.obj_arr[i];
      miss = o == -1;
      bad = !miss && (uint32_t)o >= L.n_obj;
      if (!miss && !bad) m = (int32_t)bits(S.objs[(size_t)o * 4].y);
    } else if (L.mat_arr) {
      m = L.mat_arr[i];
    }
    if (!miss && !bad) bad = (uint32_t)m >= L.n_mat;
    if (!miss && !bad) M = mats[m];
    // phong prologue, shading.hpp:66-76
    fin = vscale(mk(M.cx, M.cy, M.cz), L.ambient);
    nn = vnormalized(mk(L.normal[i3], L.normal[i3 + 1], L.normal[i3 + 2]));
    in_dn = vnormalized(mk(L.view[i3], L.view[i3 + 1], L.view[i3 + 2]));
  }

  for (uint32_t li = 0; li < n_light; ++li) {  // wave-uniform
    const DLight Lg = load_light(lights[li]);
    const LightRay lr = light_ray(Lg, hit);  // shading.hpp:79-85
    // ---- shadow_intensity, shading.hpp:22-45 ----
    float intensity = 0.0f, shadow_fac;
    float min_t = (float)(0.0 + 1e-3);  // last_hit = 0
    for (;;) {
      const Best h = cast<V, RP_THREADS, true>(S, hit, lr.dir, min_t, lr.dist, stk, opaque);
      if (!(h.obj != RQ_NONE && h.t < lr.dist)) {
        shadow_fac = intensity;
        break;
      }
      const float trans = mats[bits(S.objs[(size_t)h.obj * 4].y)].transparency;  // get_bounce_params
      intensity += (1.0f - trans);
      if (intensity >= 1.0f) {
        shadow_fac = 1.0f;
        break;
      }
      min_t = (float)((double)h.t + 1e-3);  // last_hit + 1e-3 is a double add, shading.hpp:32
    }
    if (L.light_shadow) L.light_shadow[(size_t)i * n_light + li] = shadow_fac;
    // shading.hpp:86-95
    if (want_color && shadow_fac < 1.0f) fin = vadd(fin, lit_term<EXACT>(M, Lg, nn, in_dn, lr.dir, shadow_fac));
  }

  if (want_color) {
    if (miss) fin = mk(0.f, 0.f, 0.f);
    if (bad) fin = mk(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
    L.color[i3] = fin.x; L.color[i3 + 1] = fin.y; L.color[i3 + 2] = fin.z;
  }
}

}  // namespace

size_t ctr_points_lds_bytes(const PointsLaunch &L) {
  return walk_stack_bytes(L.scene.stack_slots, RP_THREADS, (L.flags & CTR_POINTS_LINEAR) != 0);
}

int ctr_launch_points(const PointsLaunch &L, void *stream) {
  if (L.n_points == 0) return 0;
  const bool lin = (L.flags & CTR_POINTS_LINEAR) != 0, exact = (L.flags & CTR_POINTS_EXACT_POW) != 0;
  void (*const kernel)(PointsLaunch) = lin ? (exact ? ray_points_kernel<RP_LINEAR | RP_EXACT> : ray_points_kernel<RP_LINEAR>)
                                           : (exact ? ray_points_kernel<RP_EXACT> : ray_points_kernel<0u>);
  return launch_lanes(kernel, L, L.n_points, RP_THREADS, ctr_points_lds_bytes(L), (hipStream_t)stream);
}
