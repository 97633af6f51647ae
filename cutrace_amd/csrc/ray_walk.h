// ray_walk.h — the per-lane walk of the ray queries: ray_cast (inc/ray_cast.hpp:29-55) of ONE ray by ONE lane.
//
// Shared by ray_query.hip (ctr_cast_rays), ray_shade.hip (ctr_shade_rays), ray_points.hip (ctr_shade_points) and ray_hits.hip (ctr_list_hits); what each step may and may not shortcut
// is stated at the top of ray_query.hip.  Device code only: include it from a .hip translation unit, after
// hip_runtime.h.  Everything lives in an unnamed namespace, one copy per translation unit.
//
// Template arguments of cast / cast_mesh:
//   V        RQ_* bits: RQ_LINEAR walks meshes linearly; RQ_ANYHIT stops EVERY lane at the first object whose accepted
//            t lies below t_lim
//   STRIDE   lanes per workgroup: the LDS stack is laid out [entry][STRIDE], `stk` points at the lane's entry 0
//   LANE_AH  the `lane_anyhit` argument is honoured: the early-out of RQ_ANYHIT decided per lane at run time (a wave
//            whose lanes cast shadow rays and radiance rays through one call site)
#ifndef CUTRACE_AMD_RAY_WALK_H
#define CUTRACE_AMD_RAY_WALK_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "ray_query.h"
#include "scene_device.h"
#include "vec3.h"

namespace {

constexpr int RQ_THREADS = 128;  // lanes per workgroup of ray_query.hip (the default STRIDE)
enum : uint32_t { RQ_LINEAR = 1u, RQ_SHADOW = 2u, RQ_ANYHIT = 4u };
constexpr uint32_t RQ_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t bits(float x) { return __float_as_uint(x); }

// The nearest hit so far: ray_cast.hpp:43 keeps the first object in scene order among equal t, i.e. the
// lexicographic minimum of (t, object index) over the objects whose own t exceeds min_t.
struct Best {
  float t = INFINITY;
  uint32_t obj = RQ_NONE;   // object index (ctr_scene_desc.objects)
  uint32_t tri = RQ_NONE;   // DTri / gnorm record of a triangle or mesh hit (mesh: tri_begin + file index)
  uint32_t prim = RQ_NONE;  // mesh hit: the triangle's file index within the mesh
  __device__ __forceinline__ bool beaten_by(float t2, uint32_t obj2) const { return t2 < t || (t2 == t && obj2 < obj); }
};

// triangle::intersect, default_schema.hpp:57-78, against one DTri (a = p2 - p1, b = p2 - p3 hoisted at upload with the
// same operations).  True when the triangle is valid (beta, gamma in range, t0 finite, min_t <= t0) AND its t0 can
// still matter: t0 <= lim (the nearest hit so far, or max_t).  t0 is then the reference's IEEE quotient.  A 1-ulp
// reciprocal decides where its quotients clear the margins of render_kernel.hip's exact test (2^-18 relative, 2^-16 on
// beta + gamma, 1e-30 absolute): those cover its own rounding and the reference's; everything else divides.
__device__ __forceinline__ bool tri_hit(const float4 *rec, V3 ro, V3 rd, float min_t, float lim, float &t_out, uint32_t &orig) {
  const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
  const V3 a = mk(w0.x, w0.z, w1.x), b = mk(w0.y, w0.w, w1.y);
  const V3 d = mk(w1.z - ro.x, w1.w - ro.y, w2.x - ro.z);  // p2 - start
  orig = bits(w2.y);
  const float alpha = det3(a, b, rd);
  const float A1 = det3(d, b, rd), A2 = det3(a, d, rd), A0 = det3(a, b, d);
  const float r = __builtin_amdgcn_rcpf(alpha);
  const float bq = A1 * r, gq = A2 * r, tq = A0 * r, sq = bq + gq;
  const float eb = fabsf(bq) * 0x1p-18f + 1e-30f, eg = fabsf(gq) * 0x1p-18f + 1e-30f;
  const float es = (fabsf(bq) + fabsf(gq) + 1.0f) * 0x1p-16f;
  const float et = fabsf(tq) * 0x1p-18f + 1e-30f;
  if ((bq < -eb) | (gq < -eg) | (sq > 1.0f + es) | (tq < min_t - et)) return false;
  if ((bq > eb) & (gq > eg) & (sq < 1.0f - es) & (tq > min_t + et) & (fabsf(tq) < 1e37f)) {
    if (tq - et > lim) return false;  // valid, but certainly beyond anything that can still win or tie
    t_out = A0 / alpha;
    return true;
  }
  const float beta = A1 / alpha, gamma = A2 / alpha, t0 = A0 / alpha;
  t_out = t0;
  return beta >= 0 && gamma >= 0 && beta + gamma <= 1 && __builtin_isfinite(t0) && min_t <= t0;
}

struct Scene {
  const float4 *objs, *oloop, *meshes, *planes, *tris, *nodes4;  // 4, 4, 4, 4, 4 and 8 float4 per record
  const float *gnorm;
  const DMat *mats;
  uint32_t n_oloop, n_plane_recs, n_mesh, slots;
  bool ign;
};
// `ign` != 0: ray_cast's ignore_transparent
__device__ __forceinline__ Scene make_scene(const RayScene &R, uint32_t ign) {
  Scene S;
  S.objs = (const float4 *)R.objs;
  S.oloop = (const float4 *)R.oloop;
  S.meshes = (const float4 *)R.meshes;
  S.planes = (const float4 *)R.planes;
  S.tris = (const float4 *)R.tris;
  S.nodes4 = (const float4 *)R.nodes4;
  S.gnorm = R.gnorm;
  S.mats = R.mats;
  S.n_oloop = R.n_oloop;
  S.n_plane_recs = R.n_plane_recs;
  S.n_mesh = R.n_mesh;
  S.slots = R.stack_slots;
  S.ign = ign != 0u;
  return S;
}

// One mesh (a DObj record that passed the reference's AABB test): its nearest valid triangle, ties to the lower file
// index (default_schema.hpp:133-134, strict < in file order), then ray_cast.hpp:43's strict test against min_t.
//
// The BVH's box test runs on the direction scaled by a power of two to a largest component in [1, 2) (BoxRay, made once
// per cast): its distances are t * tk, and so are the two bounds it compares them with, min_t and the limit.  Scaling
// by a power of two is exact, so for a direction of any length the test decides what it decides for that direction at
// unit length; a bound that leaves the normal range on the way is moved outwards (floor_tk, ceil_tk).
struct BoxRay {
  V3 ria;    // 1-ulp reciprocals of the scaled direction, clamped to +-1e30
  float tk;  // a power of two: box distance = t * tk
};
__device__ __forceinline__ BoxRay box_ray(V3 rd) {
  const float am = fmaxf(fmaxf(fabsf(rd.x), fabsf(rd.y)), fabsf(rd.z));  // (fmaxf skips a NaN component)
  int e = 1;                                                              // am = m * 2^e, m in [0.5, 1)
  if (am > 0.0f && am < INFINITY) (void)frexpf(am, &e);                   // no finite non-zero component: unscaled
  const V3 rs = mk(ldexpf(rd.x, 1 - e), ldexpf(rd.y, 1 - e), ldexpf(rd.z, 1 - e));
  BoxRay B;
  B.ria = mk(fminf(fmaxf(__builtin_amdgcn_rcpf(rs.x), -1e30f), 1e30f), fminf(fmaxf(__builtin_amdgcn_rcpf(rs.y), -1e30f), 1e30f),
             fminf(fmaxf(__builtin_amdgcn_rcpf(rs.z), -1e30f), 1e30f));
  B.tk = ldexpf(1.0f, e - 1);  // 2^-149 .. 2^127: always representable
  return B;
}
// t * tk as a lower / an upper bound of box distances: exact unless the product is denormal, then rounded outwards.  A
// lower bound that overflows stays finite (the largest float is still below it): no box distance, which the clamped
// reciprocals keep finite, is then culled by an infinity the linear walk never sees.
__device__ __forceinline__ float floor_tk(float t, float tk) {
  const float p = fminf(t * tk, 3.4028235e38f);
  return fabsf(p) < 0x1p-126f ? (p > 0.0f ? 0.0f : -0x1p-126f) : p;
}
__device__ __forceinline__ float ceil_tk(float t, float tk) {
  const float p = t * tk;
  return fabsf(p) < 0x1p-126f ? (p < 0.0f ? 0.0f : 0x1p-126f) : p;
}

template <uint32_t V, int STRIDE = RQ_THREADS>
__device__ __forceinline__ void cast_mesh(const Scene &S, const float4 *O, V3 ro, V3 rd, const BoxRay &B, float min_t, float t_lim,
                                          Best &best, uint32_t *stk) {
  const float4 o0 = O[0], o1 = O[1], o2 = O[2], o3 = O[3];
  const uint32_t tri_begin = bits(o0.z), tri_count = bits(o0.w), node_begin = bits(o1.x), bvh_root = bits(o1.z),
                 index = bits(o1.w);
  float mt = INFINITY;
  uint32_t morig = RQ_NONE;
  float lim = fminf(best.t, t_lim);  // no triangle beyond it can win or tie
  float blim = (V & RQ_LINEAR) ? 0.0f : ceil_tk(lim, B.tk);  // `lim` as a box distance
  auto test = [&](uint32_t k) {
    float t0;
    uint32_t orig;
    if (tri_hit(S.tris + (size_t)k * 4, ro, rd, min_t, lim, t0, orig) && (t0 < mt || (t0 == mt && orig < morig))) {
      mt = t0;
      morig = orig;
      lim = fminf(lim, mt);
      if (!(V & RQ_LINEAR)) blim = ceil_tk(lim, B.tk);
    }
  };
  if (V & RQ_LINEAR) {
    for (uint32_t k = 0; k < tri_count; ++k) test(tri_begin + k);
  } else {
    // box constants of render_kernel.hip's per-mesh walk: the boxes widened by mw in world space
    const V3 ria = B.ria;
    const float bmin = floor_tk(min_t, B.tk);  // min_t as a box distance
    const float gx = fmaxf(fabsf(o2.x - ro.x), fabsf(o2.w - ro.x));
    const float gy = fmaxf(fabsf(o2.y - ro.y), fabsf(o3.x - ro.y));
    const float gz = fmaxf(fabsf(o2.z - ro.z), fabsf(o3.y - ro.z));
    // (+ 2^-21 x the origin's largest |coordinate|: (ro + mw) and its product are rounded to 2^-24 of |ro|, which for a scene far off
    //  the origin exceeds 2^-14 x the distance to the box — the walk then missed triangles; as in render_kernel.hip)
    const float mw = __builtin_fmaf(fmaxf(fmaxf(fabsf(ro.x), fabsf(ro.y)), fabsf(ro.z)), 0x1p-21f, fmaxf(fmaxf(gx, gy), gz) * 0x1p-14f);
    const V3 ka = mk((ro.x + mw) * ria.x, (ro.y + mw) * ria.y, (ro.z + mw) * ria.z);  // for box minima
    const V3 kb = mk((ro.x - mw) * ria.x, (ro.y - mw) * ria.y, (ro.z - mw) * ria.z);  // for box maxima
    const float4 *nodes = S.nodes4 + (size_t)node_begin * 8;
    const uint32_t neg = (bits(rd.x) >> 31) | ((bits(rd.y) >> 31) << 1) | ((bits(rd.z) >> 31) << 2);
    // node 0 is the root; a mesh with guard records starts at its spare node (children: the guard leaf and the root)
    uint32_t cur = bvh_root, sp = 0;
    for (;;) {
      const float4 *N = nodes + (size_t)cur * 8;
      const float4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3], q4 = N[4], q5 = N[5], q6 = N[6], q7 = N[7];
      float en[4], ex[4];
      uint32_t ch[4] = {bits(q6.x), bits(q6.y), bits(q6.z), bits(q6.w)};
#define RQ_BOX(c, F)                                                                                      \
  {                                                                                                       \
    const float t1x = __builtin_fmaf(q0.F, ria.x, -ka.x), t2x = __builtin_fmaf(q3.F, ria.x, -kb.x);      \
    const float t1y = __builtin_fmaf(q1.F, ria.y, -ka.y), t2y = __builtin_fmaf(q4.F, ria.y, -kb.y);      \
    const float t1z = __builtin_fmaf(q2.F, ria.z, -ka.z), t2z = __builtin_fmaf(q5.F, ria.z, -kb.z);      \
    en[c] = fmaxf(fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z)), bmin);               \
    ex[c] = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));                            \
  }
      RQ_BOX(0, x) RQ_BOX(1, y) RQ_BOX(2, z) RQ_BOX(3, w)
#undef RQ_BOX
      // children are stored sorted along the node's axis: a ray pointing the other way takes them in reverse
      if ((neg >> bits(q7.x)) & 1u) {
        float f;
        uint32_t u;
        f = en[0]; en[0] = en[3]; en[3] = f; f = en[1]; en[1] = en[2]; en[2] = f;
        f = ex[0]; ex[0] = ex[3]; ex[3] = f; f = ex[1]; ex[1] = ex[2]; ex[2] = f;
        u = ch[0]; ch[0] = ch[3]; ch[3] = u; u = ch[1]; ch[1] = ch[2]; ch[2] = u;
      }
      // leaves near to far (what they find prunes the rest), then the inner children: the nearest is visited next,
      // the others wait on the stack
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if ((ch[c] & BVH_LEAF_FLAG) && !(en[c] > fminf(ex[c], blim))) {
          const uint32_t first = tri_begin + (ch[c] & 0xFFFFFFu), n = (ch[c] >> 24) & 0x7Fu;
          for (uint32_t j = 0; j < n; ++j) test(first + j);
        }
      }
      uint32_t next = RQ_NONE;
#pragma unroll
      for (int c = 3; c >= 0; --c) {
        if (!(ch[c] & BVH_LEAF_FLAG) && !(en[c] > fminf(ex[c], blim))) {
          if (next != RQ_NONE && sp < S.slots) stk[(sp++) * STRIDE] = next;
          next = ch[c];
        }
      }
      if (next == RQ_NONE) {
        if (sp == 0) break;
        next = stk[(--sp) * STRIDE];
      }
      cur = next;
    }
  }
  // default_schema.hpp:143 (a hit at all), ray_cast.hpp:43 (strict > min_dist; strict < with the lower index on ties)
  if (morig != RQ_NONE && mt > min_t && best.beaten_by(mt, index)) {
    best.t = mt;
    best.obj = index;
    best.tri = tri_begin + morig;  // gnorm is indexed by the file-order position within the mesh
    best.prim = morig;
  }
}

// ray_cast (ray_cast.hpp:29-55) of one ray.  t_lim: nothing beyond it is asked for (SHADOW: max_t; else +inf).
template <uint32_t V, int STRIDE = RQ_THREADS, bool LANE_AH = false>
__device__ Best cast(const Scene &S, V3 ro, V3 rd, float min_t, float t_lim, uint32_t *stk, bool lane_anyhit = false) {
  Best best;
  const bool ANYHIT = (V & RQ_ANYHIT) != 0 || (LANE_AH && lane_anyhit);  // a constant unless LANE_AH
  // ---- planes: plane::intersect, default_schema.hpp:189-201 (two per record, coordinates interleaved) ----
  for (uint32_t p = 0; p < S.n_plane_recs; ++p) {
    const float4 *P = S.planes + (size_t)p * 4;
    const float4 w0 = P[0], w1 = P[1], w2 = P[2], w3 = P[3];
    const float px[2] = {w0.x, w0.y}, py[2] = {w0.z, w0.w}, pz[2] = {w1.x, w1.y};
    const float nx[2] = {w1.z, w1.w}, ny[2] = {w2.x, w2.y}, nz[2] = {w2.z, w2.w};
    const uint32_t idx[2] = {bits(w3.x), bits(w3.y)}, tr[2] = {bits(w3.z), bits(w3.w)};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (idx[s] == CTR_PLANE_PAD || (S.ign && tr[s])) continue;  // (ray_cast.hpp:39-40)
      const float num = ((px[s] - ro.x) * nx[s] + (py[s] - ro.y) * ny[s]) + (pz[s] - ro.z) * nz[s];
      const float den = (rd.x * nx[s] + rd.y * ny[s]) + rd.z * nz[s];
      const float t0 = num / den;
      // isfinite && min_t <= t0 (plane) && t0 > min_t (ray_cast.hpp:43)
      if (__builtin_isfinite(t0) && t0 > min_t && best.beaten_by(t0, idx[s])) {
        best.t = t0;
        best.obj = idx[s];
        best.tri = RQ_NONE;
        best.prim = RQ_NONE;
      }
    }
  }
  if (ANYHIT && best.t < t_lim) return best;
  // ---- spheres and stand-alone triangles, scene order ----
  V3 sd = mk(0, 0, 0);  // sphere::intersect's normalised direction (default_schema.hpp:227), made at the first sphere
  float sdd = 0.f;
  bool have_sd = false;
  for (uint32_t i = 0; i < S.n_oloop; ++i) {
    const float4 *O = S.oloop + (size_t)i * 4;
    const float4 o0 = O[0], o1 = O[1], o2 = O[2], o3 = O[3];
    if (S.ign && bits(o3.w)) continue;
    const uint32_t index = bits(o1.w);
    bool ok;
    float cand = INFINITY;
    uint32_t ctri = RQ_NONE;
    if (bits(o0.x) == CTR_OBJ_SPHERE) {
      // ---- sphere::intersect, default_schema.hpp:226-251 ----
      if (!have_sd) {
        sd = vnormalized(rd);
        sdd = vdot(sd, sd);
        have_sd = true;
      }
      const V3 ec = vsub(ro, mk(o2.x, o2.y, o2.z));
      const float R = o2.w;
      const float dec = -vdot(sd, ec);
      const float sub = dec * dec - sdd * (vdot(ec, ec) - R * R);
      const float sq = sqrtf(sub);
      const float t0 = (dec - sq) / sdd, t1 = (dec + sq) / sdd;
      const bool t0v = __builtin_isfinite(t0) && min_t <= t0, t1v = __builtin_isfinite(t1) && min_t <= t1;
      ok = t0v || t1v;
      cand = (t0v && t1v) ? smin(t0, t1) : (t0v ? t0 : t1);
    } else {
      uint32_t unused;
      ctri = bits(o0.z);
      ok = tri_hit(S.tris + (size_t)ctri * 4, ro, rd, min_t, fminf(best.t, t_lim), cand, unused);
    }
    // ray_cast.hpp:43 — strict >, strict < with the first object in scene order winning ties
    if (ok && cand > min_t && best.beaten_by(cand, index)) {
      best.t = cand;
      best.obj = index;
      best.tri = ctri;
      best.prim = RQ_NONE;
    }
    if (ANYHIT && best.t < t_lim) return best;
  }
  // ---- meshes ----
  if (S.n_mesh != 0u) {
    const V3 rinv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);  // default_schema.hpp:103
    // the BVH's box test: 1-ulp reciprocals of the direction at unit scale, clamped to +-1e30 (an axis-parallel ray gets
    // huge finite slab distances)
    BoxRay B;
    B.ria = mk(0, 0, 0);
    B.tk = 1.0f;
    if (!(V & RQ_LINEAR)) B = box_ray(rd);
    for (uint32_t m = 0; m < S.n_mesh; ++m) {
      const float4 *O = S.meshes + (size_t)m * 4;
      const float4 o2 = O[2], o3 = O[3];
      if (S.ign && bits(o3.w)) continue;
      // ---- mesh::bound_intersects, default_schema.hpp:99-114 ----
      float tmin = 0.0f, tmax = INFINITY;
      float t1 = (o2.x - ro.x) * rinv.x, t2 = (o2.w - ro.x) * rinv.x;
      tmin = smin(smax(t1, tmin), smax(t2, tmin));
      tmax = smax(smin(t1, tmax), smin(t2, tmax));
      t1 = (o2.y - ro.y) * rinv.y; t2 = (o3.x - ro.y) * rinv.y;
      tmin = smin(smax(t1, tmin), smax(t2, tmin));
      tmax = smax(smin(t1, tmax), smin(t2, tmax));
      t1 = (o2.z - ro.z) * rinv.z; t2 = (o3.y - ro.z) * rinv.z;
      tmin = smin(smax(t1, tmin), smax(t2, tmin));
      tmax = smax(smin(t1, tmax), smin(t2, tmax));
      if (!(tmin <= tmax)) continue;
      cast_mesh<V, STRIDE>(S, O, ro, rd, B, min_t, t_lim, best, stk);
      if (ANYHIT && best.t < t_lim) return best;
    }
  }
  return best;
}

}  // namespace

#endif
