// ray_cross.hip — the kernels behind ctr_count_crossings and ctr_inside_points (include/cutrace_inside.h): how many surfaces a
// ray crosses, and with that whether a point lies inside a body.
//
// ONE LANE = ONE RAY (ray_cross_kernel) or ONE POINT (ray_inside_kernel), RQ_THREADS lanes per workgroup, the launch record as the
// one argument, the scene as the ray queries describe it (RayScene) and their per-lane LDS stack laid out [entry][lane]
// (ray_walk.h, walk_stack_bytes).  The header is the definition: the count is a SUM over the selected primitives of terms each
// primitive decides alone, so this file is only the order of the visits, which cannot change the answer.
//
// The walk is NOT cast<V> (ray_walk.h): that one looks for the nearest hit and lets every hit it finds shorten the ray.  Here
// NOTHING PRUNES ON DISTANCE.  The two box limits are fixed for the whole walk, bmin = floor_tk(min_t) and blim = ceil_tk(max_t);
// a triangle is tri_hit (ray_walk.h) with lim = max_t — the reference's test, and a drop only of what lies certainly beyond max_t —
// followed by the exact t0 > min_t && t0 < max_t.  The box arithmetic is cast_mesh's, operation for operation: BoxRay, the margin
// mw, ka / kb and the fma slabs.  Children need neither sorting nor reversal: the leaves of every admitted child are tested, the
// admitted inner children are pushed (at most three per node wait while the fourth is visited: FlatScene::ray_slots, as the cast).
//
// A mesh is walked from node 0, the ROOT, never from DObj::bvh_root (the rule at the top of ray_nearest.hip): a mesh with guard
// records starts its RAY walk at a spare node whose guard leaf holds COPIES of triangles the tree under node 0 holds already — a
// count from there counts them twice — and a mesh the ray walk takes linearly keeps its tree with every used box unbounded, which
// from node 0 is every triangle once with nothing culled.  node_count == 0 is the linear loop.  The mesh's own box
// (bound_intersects) is not looked at: it is not part of the definition.
//
// ray_inside_kernel: the R directions are the same for every lane — scalar data, read from the launch record — so the wave takes
// direction r in lock step, BoxRay and the sphere's unit direction are made once per direction, and neighbouring points send
// neighbouring PARALLEL rays through the tree.  Without d_votes a wave leaves the loop after the first direction at which a
// ballot shows every one of its points decided (more than half of R odd, or more than half even).  No scratch memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "cutrace_inside.h"
#include "ray_cross.h"
#include "ray_launch.h"
#include "ray_walk.h"
#include "scene_device.h"

namespace {

// the two sums of one ray
struct Cross {
  int32_t n = 0;  // the crossing count
  int32_t s = 0;  // the signed count
};

__device__ __forceinline__ bool finite3(V3 v) { return fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY && fabsf(v.z) < INFINITY; }

// one triangle record's term
__device__ __forceinline__ void cross_tri(const float4 *rec, V3 ro, V3 rd, float min_t, float max_t, Cross &c) {
  float t0;
  uint32_t unused;
  if (tri_hit(rec, ro, rd, min_t, max_t, t0, unused) && t0 > min_t && t0 < max_t) {
    const float4 w0 = rec[0], w1 = rec[1];
    const float alpha = det3(mk(w0.x, w0.z, w1.x), mk(w0.y, w0.w, w1.y), rd);  // tri_hit's: a finite t0 has alpha != 0
    c.n += 1;
    c.s += alpha < 0.0f ? 1 : -1;
  }
}

// one mesh's terms
template <bool LINEAR, int STRIDE = RQ_THREADS>
__device__ __forceinline__ void cross_mesh(const Scene &S, const float4 *O, V3 ro, V3 rd, const BoxRay &B, float min_t, float max_t,
                                           Cross &c, uint32_t *stk) {
  const float4 o0 = O[0], o1 = O[1], o2 = O[2], o3 = O[3];
  const uint32_t tri_begin = bits(o0.z), tri_count = bits(o0.w), node_begin = bits(o1.x), node_count = bits(o1.y);
  if (LINEAR || node_count == 0u) {
    for (uint32_t k = 0; k < tri_count; ++k) cross_tri(S.tris + (size_t)(tri_begin + k) * 4, ro, rd, min_t, max_t, c);
    return;
  }
  // the box constants of cast_mesh (ray_walk.h); the limits never move
  const V3 ria = B.ria;
  const float bmin = floor_tk(min_t, B.tk), blim = ceil_tk(max_t, B.tk);
  const float gx = fmaxf(fabsf(o2.x - ro.x), fabsf(o2.w - ro.x));
  const float gy = fmaxf(fabsf(o2.y - ro.y), fabsf(o3.x - ro.y));
  const float gz = fmaxf(fabsf(o2.z - ro.z), fabsf(o3.y - ro.z));
  const float mw = __builtin_fmaf(fmaxf(fmaxf(fabsf(ro.x), fabsf(ro.y)), fabsf(ro.z)), 0x1p-21f, fmaxf(fmaxf(gx, gy), gz) * 0x1p-14f);
  const V3 ka = mk((ro.x + mw) * ria.x, (ro.y + mw) * ria.y, (ro.z + mw) * ria.z);  // for box minima
  const V3 kb = mk((ro.x - mw) * ria.x, (ro.y - mw) * ria.y, (ro.z - mw) * ria.z);  // for box maxima
  const float4 *nodes = S.nodes4 + (size_t)node_begin * 8;
  uint32_t cur = 0, sp = 0;  // node 0: the root
  for (;;) {
    const float4 *N = nodes + (size_t)cur * 8;
    const float4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3], q4 = N[4], q5 = N[5], q6 = N[6];
    uint32_t next = RQ_NONE;
#define CR_CHILD(F)                                                                                      \
  {                                                                                                       \
    const float t1x = __builtin_fmaf(q0.F, ria.x, -ka.x), t2x = __builtin_fmaf(q3.F, ria.x, -kb.x);      \
    const float t1y = __builtin_fmaf(q1.F, ria.y, -ka.y), t2y = __builtin_fmaf(q4.F, ria.y, -kb.y);      \
    const float t1z = __builtin_fmaf(q2.F, ria.z, -ka.z), t2z = __builtin_fmaf(q5.F, ria.z, -kb.z);      \
    const float en = fmaxf(fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z)), bmin);       \
    const float ex = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));                    \
    const uint32_t ch = bits(q6.F);                                                                       \
    if (!(en > fminf(ex, blim))) {                                                                        \
      if (ch & BVH_LEAF_FLAG) {                                                                           \
        const uint32_t first = tri_begin + (ch & 0xFFFFFFu), n = (ch >> 24) & 0x7Fu;                      \
        for (uint32_t j = 0; j < n; ++j) cross_tri(S.tris + (size_t)(first + j) * 4, ro, rd, min_t, max_t, c); \
      } else {                                                                                            \
        if (next != RQ_NONE && sp < S.slots) stk[(sp++) * STRIDE] = next;                                 \
        next = ch;                                                                                        \
      }                                                                                                   \
    }                                                                                                     \
  }
    CR_CHILD(x) CR_CHILD(y) CR_CHILD(z) CR_CHILD(w)
#undef CR_CHILD
    if (next == RQ_NONE) {
      if (sp == 0) break;
      next = stk[(--sp) * STRIDE];
    }
    cur = next;
  }
}

// sphere::intersect's two roots (default_schema.hpp:226-251) along sd = d / |d|, sdd = sd . sd
__device__ __forceinline__ void cross_sphere(float4 o2, V3 ro, V3 sd, float sdd, float min_t, float max_t, Cross &c) {
  const V3 ec = vsub(ro, mk(o2.x, o2.y, o2.z));
  const float R = o2.w;
  const float dec = -vdot(sd, ec);
  const float sub = dec * dec - sdd * (vdot(ec, ec) - R * R);
  const float sq = sqrtf(sub);
  const float t0 = (dec - sq) / sdd, t1 = (dec + sq) / sdd;
  if (__builtin_isfinite(t0) && t0 > min_t && t0 < max_t) { c.n += 1; c.s -= 1; }
  if (__builtin_isfinite(t1) && t1 > min_t && t1 < max_t) { c.n += 1; c.s += 1; }
}

// Every selected primitive's term for one ray.  SOLIDS: meshes and spheres only (ctr_inside_points), the planes' and the stand-alone
// triangles' code is not compiled.  `only`: RQ_NONE, or the one object counted.  B: box_ray(rd), unused by a LINEAR walk.
template <bool LINEAR, bool SOLIDS>
__device__ __forceinline__ Cross cross_ray(const Scene &S, V3 ro, V3 rd, V3 sd, float sdd, const BoxRay &B, float min_t, float max_t,
                                           uint32_t only, uint32_t flags, uint32_t *stk) {
  Cross c;
  // ---- planes: plane::intersect, default_schema.hpp:189-201 (two per record, coordinates interleaved) ----
  if (!SOLIDS && !(flags & CTR_CROSS_SKIP_PLANES)) {
    for (uint32_t p = 0; p < S.n_plane_recs; ++p) {
      const float4 *P = S.planes + (size_t)p * 4;
      const float4 w0 = P[0], w1 = P[1], w2 = P[2], w3 = P[3];
      const float px[2] = {w0.x, w0.y}, py[2] = {w0.z, w0.w}, pz[2] = {w1.x, w1.y};
      const float nx[2] = {w1.z, w1.w}, ny[2] = {w2.x, w2.y}, nz[2] = {w2.z, w2.w};
      const uint32_t idx[2] = {bits(w3.x), bits(w3.y)};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (idx[s] == CTR_PLANE_PAD || (only != RQ_NONE && idx[s] != only)) continue;
        const float num = ((px[s] - ro.x) * nx[s] + (py[s] - ro.y) * ny[s]) + (pz[s] - ro.z) * nz[s];
        const float den = (rd.x * nx[s] + rd.y * ny[s]) + rd.z * nz[s];
        const float t0 = num / den;
        if (__builtin_isfinite(t0) && t0 > min_t && t0 < max_t) {
          c.n += 1;
          c.s += den > 0.0f ? 1 : -1;
        }
      }
    }
  }
  // ---- spheres and stand-alone triangles, scene order ----
  for (uint32_t i = 0; i < S.n_oloop; ++i) {
    const float4 *O = S.oloop + (size_t)i * 4;
    const float4 o0 = O[0], o1 = O[1], o2 = O[2];
    if (only != RQ_NONE && bits(o1.w) != only) continue;
    if (bits(o0.x) == CTR_OBJ_SPHERE) cross_sphere(o2, ro, sd, sdd, min_t, max_t, c);
    else if (!SOLIDS && !(flags & CTR_CROSS_SKIP_TRIANGLES)) cross_tri(S.tris + (size_t)bits(o0.z) * 4, ro, rd, min_t, max_t, c);
  }
  // ---- meshes ----
  for (uint32_t m = 0; m < S.n_mesh; ++m) {
    const float4 *O = S.meshes + (size_t)m * 4;
    if (only != RQ_NONE && bits(O[1].w) != only) continue;
    cross_mesh<LINEAR>(S, O, ro, rd, B, min_t, max_t, c, stk);
  }
  return c;
}

__device__ __forceinline__ BoxRay no_box_ray() {
  BoxRay B;
  B.ria = mk(0, 0, 0);
  B.tk = 1.0f;
  return B;
}

template <bool LINEAR>
__global__ __launch_bounds__(RQ_THREADS) void ray_cross_kernel(CrossLaunch L) {
  extern __shared__ uint32_t rq_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RQ_THREADS + threadIdx.x;
  if (i >= L.n_rays) return;
  const Scene S = make_scene(L.scene, 0u);
  uint32_t *stk = rq_stack + threadIdx.x;
  const size_t i3 = (size_t)i * 3;
  const V3 ro = mk(L.origin[i3], L.origin[i3 + 1], L.origin[i3 + 2]);
  const V3 rd = mk(L.dir[i3], L.dir[i3 + 1], L.dir[i3 + 2]);
  const float min_t = L.min_t_arr ? L.min_t_arr[i] : L.min_t;
  const float max_t = L.max_t_arr ? L.max_t_arr[i] : L.max_t;
  Cross c;
  // a ray that is not one: 0 / 0
  if (finite3(ro) && finite3(rd) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f)) {
    const V3 sd = vnormalized(rd);  // sphere::intersect's direction (default_schema.hpp:227)
    c = cross_ray<LINEAR, false>(S, ro, rd, sd, vdot(sd, sd), LINEAR ? no_box_ray() : box_ray(rd), min_t, max_t, (uint32_t)L.only, L.flags, stk);
  }
  if (L.count) L.count[i] = c.n;
  if (L.sgn) L.sgn[i] = c.s;
}

template <bool LINEAR>
__global__ __launch_bounds__(RQ_THREADS) void ray_inside_kernel(InsideLaunch L) {
  extern __shared__ uint32_t rq_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RQ_THREADS + threadIdx.x;
  if (i >= L.n_points) return;
  const Scene S = make_scene(L.scene, 0u);
  uint32_t *stk = rq_stack + threadIdx.x;
  const size_t i3 = (size_t)i * 3;
  const V3 p = mk(L.point[i3], L.point[i3 + 1], L.point[i3 + 2]);
  const bool live = finite3(p);  // a point that is not one: no votes
  const uint32_t R = L.n_dirs;
  const bool all_rays = L.votes != nullptr;
  uint32_t odd = 0;
  for (uint32_t r = 0; r < R; ++r) {  // the same r in every lane
    const V3 rd = mk(L.dirs[r * 3], L.dirs[r * 3 + 1], L.dirs[r * 3 + 2]);
    const V3 sd = vnormalized(rd);
    if (live) {
      const Cross c = cross_ray<LINEAR, true>(S, p, rd, sd, vdot(sd, sd), LINEAR ? no_box_ray() : box_ray(rd), 0.0f, INFINITY,
                                              (uint32_t)L.only, 0u, stk);
      odd += (uint32_t)c.n & 1u;
    }
    // decided: the rays left cannot change which side of R / 2 the votes end on
    const bool open = live && 2u * odd <= R && 2u * (r + 1u - odd) <= R;
    if (!all_rays && __ballot(open) == 0ull) break;
  }
  const bool in = 2u * odd > R;
  if (L.inside) L.inside[i] = in ? 1 : 0;
  if (L.votes) L.votes[i] = (uint8_t)odd;
  if (L.distance && in) {
    const float d = L.distance[i];
    if (fabsf(d) < INFINITY) L.distance[i] = -d;  // an infinite distance (nothing within max_dist) has no sign; nor has a NaN
  }
}

}  // namespace

int ctr_launch_cross(const CrossLaunch &L, void *stream) {
  if (L.n_rays == 0) return 0;
  const bool lin = (L.flags & CTR_CROSS_LINEAR) != 0;
  void (*kernel)(CrossLaunch) = lin ? ray_cross_kernel<true> : ray_cross_kernel<false>;
  return launch_lanes(kernel, L, L.n_rays, RQ_THREADS, walk_stack_bytes(L.scene.stack_slots, RQ_THREADS, lin), (hipStream_t)stream);
}

int ctr_launch_inside(const InsideLaunch &L, void *stream) {
  if (L.n_points == 0) return 0;
  const bool lin = (L.flags & CTR_INSIDE_LINEAR) != 0;
  void (*kernel)(InsideLaunch) = lin ? ray_inside_kernel<true> : ray_inside_kernel<false>;
  return launch_lanes(kernel, L, L.n_points, RQ_THREADS, walk_stack_bytes(L.scene.stack_slots, RQ_THREADS, lin), (hipStream_t)stream);
}
