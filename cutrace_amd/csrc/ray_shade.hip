// ray_shade.hip — the kernel behind ctr_shade_rays (include/cutrace_rays.h): ray_color of rays from memory.
//
// What it restates (reference, file:line), operation for operation, with the render kernel's numerics
// (render_kernel.hip "Numerics"; -ffp-contract=off, IEEE division and square root):
//   ray_color           inc/shading.hpp:116-154     the first cast, phong, reflection and transparency to `bounces`
//   phong               inc/shading.hpp:64-99       ambient + per light: shadow ray, diffuse and specular terms
//   shadow_intensity    inc/shading.hpp:22-45       a loop of nearest casts from (float)((double)last_hit + 1e-3)
// on top of the per-lane walk of ray_walk.h (ray_cast and everything below it).
//
// ONE LANE = ONE RAY for the whole life of its ray_color activation tree.  The recursion is a state machine per lane
// (the render kernel's, render_kernel.hip "continuation"): every trip of the loop makes ONE cast — a radiance cast
// (ray_color's ray_cast, shading.hpp:123) or one iteration of a light's shadow loop (shading.hpp:32) — through ONE call
// site, with the lane's own min_t, limit and (all-opaque scenes) any-hit early-out, so a wave whose lanes are in
// different states still walks together.  What comes back is consumed, and the lane's next cast prepared, by the
// straight-line code after it.
//
// Suspended activations live in LDS, [frame][field][lane] behind the walk's stack ([entry][lane]): the colour so far
// and the material (4 dwords); where some material both reflects and transmits, also the hit point and the incoming
// direction for the pass-through child that is cast after the reflection returns (10 dwords).  A frame is pushed per
// level below the first, so `bounces` frames are all a lane can need.  No scratch memory.
//
// The specular term: by default the render's fast path (1-ulp v_rsq_f32 for the half vector, exp2(e * log2(x)) on the
// transcendental pipe, phong_exp == 0 -> 1); CTR_SHADE_EXACT_POW: IEEE normalisation and f64 pow rounded once, the
// render's CTR_VAR_EXACT_POW.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "cutrace_rays.h"
#include "phong_light.h"
#include "ray_launch.h"
#include "ray_shade.h"
#include "ray_walk.h"

namespace {

constexpr int RS_THREADS = 64;  // one wave per workgroup: bounces = 15 with 10-dword frames fits a workgroup's LDS
enum : uint32_t { RS_LINEAR = 1u, RS_EXACT = 2u };
enum { F_R = 0, F_G, F_B, F_MAT, F_PX, F_PY, F_PZ, F_DX, F_DY, F_DZ };
enum { ACT_CAST = 0, ACT_LIGHT, ACT_BOUNCE, ACT_UNWIND };

__device__ __forceinline__ void store3(float *p, size_t i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

template <uint32_t K>
__global__ __launch_bounds__(RS_THREADS) void ray_shade_kernel(ShadeLaunch L) {
  constexpr uint32_t V = (K & RS_LINEAR) ? RQ_LINEAR : 0u;
  constexpr bool EXACT = (K & RS_EXACT) != 0;
  extern __shared__ uint32_t rs_lds[];
  const uint32_t i = blockIdx.x * (uint32_t)RS_THREADS + threadIdx.x;
  if (i >= L.n_rays) return;
  const Scene S = make_scene(L.scene, 0u);  // every cast of ray_color, phong and shadow_intensity passes ignore_transparent = false
  uint32_t *const stk = rs_lds + threadIdx.x;
  float *const frm = (float *)(rs_lds + ((V & RQ_LINEAR) ? 0u : L.scene.stack_slots * (uint32_t)RS_THREADS)) + threadIdx.x;
  const uint32_t fd = L.frame_dwords;
#define FRM(sp, f) frm[((uint32_t)(sp) * fd + (uint32_t)(f)) * (uint32_t)RS_THREADS]
  const DMat *const mats = L.scene.mats;
  const DLight *const lights = L.lights;
  const uint32_t n_light = L.n_light;
  const bool opaque = L.all_opaque != 0u;
  const int bounces = L.bounces;
  const float ambient = L.ambient, fudge = L.min_t;

  const size_t i3 = (size_t)i * 3;
  // the cast of the next trip
  V3 ro = mk(L.origin[i3], L.origin[i3 + 1], L.origin[i3 + 2]);
  V3 rd = mk(L.dir[i3], L.dir[i3 + 1], L.dir[i3 + 2]);
  float min_t = fudge, t_lim = INFINITY;
  bool shadow = false;
  // the running ray_color activation (its callers are in the frames below `depth`)
  int depth = 0;
  V3 in_d = rd;                                     // incoming->dir
  V3 in_dn = mk(0, 0, 0), nn = mk(0, 0, 0);         // incoming->dir.normalized(), normal.normalized()
  V3 pos = mk(0, 0, 0);                             // incoming->start + distance * incoming->dir
  V3 fin = mk(0, 0, 0), out_rgb = mk(0, 0, 0);      // phong's `final`; the colour an activation returns
  uint32_t mat_i = 0, li = 0;
  float intensity = 0.0f, light_dist = 0.0f;
  bool first = true;

  for (;;) {
    const Best h = cast<V, RS_THREADS, true>(S, ro, rd, min_t, t_lim, stk, shadow && opaque);
    const bool was_hit = h.obj != RQ_NONE;
    int act = ACT_CAST;
    if (!shadow) {
      // ---- ray_color's cast came back (shading.hpp:123): the hit record (ray_cast.hpp:44-47) ----
      V3 normal = mk(0, 0, 0);
      if (was_hit) {
        const float4 *H = S.objs + (size_t)h.obj * 4;
        const float4 h0 = H[0], h2 = H[2], h3 = H[3];
        const uint32_t type = bits(h0.x);
        mat_i = bits(h0.y);
        pos = vadd(ro, vscale(in_d, h.t));  // start + dist*dir (shading.hpp:133,143), a sphere's too
        in_dn = vnormalized(in_d);
        if (type == CTR_OBJ_SPHERE) {
          // default_schema.hpp:245-246: the hit uses the NORMALISED direction
          const V3 hit = vadd(ro, vscale(in_dn, h.t));
          normal = vnormalized(vsub(hit, mk(h2.x, h2.y, h2.z)));
          ro = hit;
        } else if (type == CTR_OBJ_PLANE) {
          ro = pos;
          normal = mk(h2.w, h3.x, h3.y);
        } else {
          ro = pos;
          const float *g = S.gnorm + (size_t)h.tri * 4;
          normal = mk(g[0], g[1], g[2]);
        }
      }
      if (first) {  // the hit of the FIRST cast
        if (L.t) L.t[i] = h.t;
        if (L.object) L.object[i] = was_hit ? (int32_t)h.obj : -1;
        if (L.normal) store3(L.normal, i, normal);
        first = false;
      }
      if (!was_hit) {
        out_rgb = mk(0.f, 0.f, 0.f);  // shading.hpp:119
        act = ACT_UNWIND;
      } else {
        // phong prologue, shading.hpp:66-76
        const DMat M = mats[mat_i];
        fin = vscale(mk(M.cx, M.cy, M.cz), ambient);
        nn = vnormalized(normal);
        li = 0;
        act = ACT_LIGHT;
      }
    } else {
      // ---- one iteration of shadow_intensity's loop, shading.hpp:32-42 ----
      bool done_shadow;
      float shadow_fac = 0.f;
      if (was_hit && h.t < light_dist) {
        const float trans = mats[bits(S.objs[(size_t)h.obj * 4].y)].transparency;  // get_bounce_params
        intensity += (1.0f - trans);
        if (intensity >= 1.0f) {
          shadow_fac = 1.0f;
          done_shadow = true;
        } else {
          min_t = (float)((double)h.t + 1e-3);  // last_hit + 1e-3 is a double add, shading.hpp:32
          done_shadow = false;                  // cast again (same ray)
        }
      } else {
        shadow_fac = intensity;
        done_shadow = true;
      }
      if (done_shadow) {
        if (shadow_fac < 1.0f) {
          // shading.hpp:86-95 (phong_light.h); the shadow ray's direction IS direction.normalized()
          fin = vadd(fin, lit_term<EXACT>(mats[mat_i], lights[li], nn, in_dn, rd, shadow_fac));
        }
        li++;
        act = ACT_LIGHT;
      }
    }

    if (act == ACT_LIGHT) {
      if (li < n_light) {
        // shading.hpp:79-85: direction and distance to light li, the shadow ray from *hit (ro) (phong_light.h)
        const LightRay lr = light_ray(lights[li], ro);
        rd = lr.dir;
        light_dist = lr.dist;
        intensity = 0.0f;
        min_t = (float)(0.0 + 1e-3);  // last_hit = 0
        t_lim = light_dist;
        shadow = true;
      } else {
        act = ACT_BOUNCE;  // phong returned `fin`
      }
    }

    if (act == ACT_BOUNCE) {
      // shading.hpp:126-150 with rgb = fin
      const DMat M = mats[mat_i];
      const bool more = depth < bounces;  // `if constexpr (bounces != 0)`
      const bool do_refl = more && (double)M.reflexivity >= 1e-6;
      const bool do_trans = more && (double)M.transparency >= 1e-6;
      if (do_refl || do_trans) {
        // push a frame, cast the child
        FRM(depth, F_R) = fin.x; FRM(depth, F_G) = fin.y; FRM(depth, F_B) = fin.z;
        FRM(depth, F_MAT) = __uint_as_float(mat_i | (do_refl ? 1u << 30 : 2u << 30));
        if (do_refl && do_trans) {  // the pass-through child is cast after the reflection returns
          FRM(depth, F_PX) = pos.x; FRM(depth, F_PY) = pos.y; FRM(depth, F_PZ) = pos.z;
          FRM(depth, F_DX) = in_d.x; FRM(depth, F_DY) = in_d.y; FRM(depth, F_DZ) = in_d.z;
        }
        depth++;
        // reflect(nd, nn) = nd - (2*(nn.nd))*nn, vector.hpp:204-206; the pass-through child keeps incoming->dir
        if (do_refl) in_d = vsub(in_dn, vscale(nn, 2.0f * vdot(nn, in_dn)));
        ro = pos; rd = in_d;
        min_t = fudge; t_lim = INFINITY;
        shadow = false;
      } else {
        out_rgb = fin;
        act = ACT_UNWIND;
      }
    }

    if (act == ACT_UNWIND) {
      // return `out_rgb` to the suspended callers
      bool done = false;
      for (;;) {
        if (depth == 0) {
          done = true;
          break;
        }
        --depth;
        V3 rgb = mk(FRM(depth, F_R), FRM(depth, F_G), FRM(depth, F_B));
        const uint32_t f_mat = __float_as_uint(FRM(depth, F_MAT));
        const DMat FM = mats[f_mat & 0x3FFFFFFFu];
        if ((f_mat >> 30) == 1u) {
          rgb = vadd(rgb, vscale(out_rgb, FM.reflexivity));  // shading.hpp:138
          if ((double)FM.transparency >= 1e-6) {
            // the frame stays, now waiting for its pass-through child (shading.hpp:141-147)
            FRM(depth, F_R) = rgb.x; FRM(depth, F_G) = rgb.y; FRM(depth, F_B) = rgb.z;
            FRM(depth, F_MAT) = __uint_as_float((f_mat & 0x3FFFFFFFu) | (2u << 30));
            in_d = mk(FRM(depth, F_DX), FRM(depth, F_DY), FRM(depth, F_DZ));
            ro = mk(FRM(depth, F_PX), FRM(depth, F_PY), FRM(depth, F_PZ));
            rd = in_d;
            depth++;
            min_t = fudge; t_lim = INFINITY;
            shadow = false;
            break;
          }
          out_rgb = rgb;
        } else {
          // shading.hpp:148
          out_rgb = vadd(vscale(rgb, 1.0f - FM.transparency), vscale(out_rgb, FM.transparency));
        }
      }
      if (done) break;
    }
  }
#undef FRM
  store3(L.color, i, out_rgb);
}

}  // namespace

size_t ctr_shade_lds_bytes(const ShadeLaunch &L) {
  return walk_stack_bytes(L.scene.stack_slots, RS_THREADS, (L.flags & CTR_SHADE_LINEAR) != 0) +
         (size_t)L.frames * L.frame_dwords * RS_THREADS * sizeof(uint32_t);
}

int ctr_launch_shade(const ShadeLaunch &L, void *stream) {
  if (L.n_rays == 0) return 0;
  const bool lin = (L.flags & CTR_SHADE_LINEAR) != 0, exact = (L.flags & CTR_SHADE_EXACT_POW) != 0;
  void (*const kernel)(ShadeLaunch) = lin ? (exact ? ray_shade_kernel<RS_LINEAR | RS_EXACT> : ray_shade_kernel<RS_LINEAR>)
                                          : (exact ? ray_shade_kernel<RS_EXACT> : ray_shade_kernel<0u>);
  return launch_lanes(kernel, L, L.n_rays, RS_THREADS, ctr_shade_lds_bytes(L), (hipStream_t)stream);
}
