// ray_nearest.hip — the kernel behind ctr_nearest_points (include/cutrace_nearest.h): the closest surface point to each point.
//
// ONE LANE = ONE POINT, RQ_THREADS lanes per workgroup, the launch record as the one argument, the scene as the ray queries
// describe it (RayScene) and their per-lane LDS stack laid out [entry][lane] (ray_walk.h, walk_stack_bytes).  What a candidate
// is, which one wins and what the cull may drop is nearest_point.h, compiled here for the device; this file is the order of
// the visits, which that definition makes irrelevant to the answer.
//
// Planes, then spheres and stand-alone triangles, then meshes: linear loops over the candidate functions.  A mesh whose box is
// farther than the best candidate so far is skipped; otherwise its tree is walked from node 0, the ROOT.  Never from
// DObj::bvh_root: a mesh with guard records starts its ray walk at the spare node, whose guard leaf holds COPIES of triangles
// the tree under node 0 holds already (guard.cpp apply_mesh copies tris[tri_begin + risky[k]], it moves nothing), and a mesh
// the ray walk takes linearly keeps its tree with every used box unbounded (guard.cpp apply_guards): under node 0 every
// triangle of the mesh is found exactly once whatever the guard state, there with nothing culled.
//
// At a node: the four children's margined bounds (np_box_bound), ordered by a fixed compare-exchange network on named registers
// (a runtime-indexed array would live in scratch memory); leaves nearest first — what they find prunes the rest — then the
// inner children: the nearest is visited next, the others wait on the stack nearer-on-top, at most three pushes per level
// (FlatScene::ray_slots).  A child is dropped only when its bound is STRICTLY above the best d2 of this mesh so far.
//
// CTR_NEAREST_LINEAR tests every record of every admitted mesh in storage (leaf) order, which with the tie rule on the file
// index is the walk in file order; no mesh is skipped and no box is looked at.  No scratch memory in either build.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "cutrace_nearest.h"
#include "nearest_point.h"
#include "ray_launch.h"
#include "ray_nearest.h"
#include "ray_walk.h"
#include "scene_device.h"

namespace {

// the nearest candidate so far: the lexicographic minimum of (d2, object index); d2 starts at the limit, obj at RQ_NONE, so
// that a candidate AT the limit still counts
struct Near {
  float d2;
  uint32_t obj = RQ_NONE;
  uint32_t rec = RQ_NONE;   // triangle or mesh: the winner's DTri record
  uint32_t gn = RQ_NONE;    // ... and its gnorm record (a mesh keeps its normals in file order)
  uint32_t prim = RQ_NONE;  // mesh: the winner's file index
  __device__ __forceinline__ bool beaten_by(float c, uint32_t obj2) const { return c < INFINITY && (c < d2 || (c == d2 && obj2 < obj)); }
};

__device__ __forceinline__ NpCand tri_cand(const float4 *rec, V3 p, uint32_t &orig) {
  const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
  orig = bits(w2.y);
  return np_triangle(w0.x, w0.z, w1.x, w0.y, w0.w, w1.y, w1.z, w1.w, w2.x, p.x, p.y, p.z);
}

template <bool LINEAR, int STRIDE = RQ_THREADS>
__device__ __forceinline__ void nearest_mesh(const Scene &S, const float4 *O, V3 p, Near &best, uint32_t *stk) {
  const float4 o0 = O[0], o1 = O[1], o2 = O[2], o3 = O[3];
  const uint32_t tri_begin = bits(o0.z), tri_count = bits(o0.w), node_begin = bits(o1.x), node_count = bits(o1.y), index = bits(o1.w);
  float md2 = best.d2;  // of this mesh: the minimum of (d2, file index) among what can still win or tie
  uint32_t morig = RQ_NONE, mrec = RQ_NONE;
  auto test = [&](uint32_t k) {
    uint32_t orig;
    const NpCand c = tri_cand(S.tris + (size_t)k * 4, p, orig);
    if (c.d2 < INFINITY && (c.d2 < md2 || (c.d2 == md2 && orig < morig))) {
      md2 = c.d2;
      morig = orig;
      mrec = k;
    }
  };
  if (LINEAR || node_count == 0u) {
    for (uint32_t k = 0; k < tri_count; ++k) test(tri_begin + k);
  } else {
    const float mw = np_margin(p.x, p.y, p.z, o2.x, o2.y, o2.z, o2.w, o3.x, o3.y);
    if (np_box_bound(o2.x, o2.y, o2.z, o2.w, o3.x, o3.y, p.x, p.y, p.z, mw) > md2) return;
    const float4 *nodes = S.nodes4 + (size_t)node_begin * 8;
    uint32_t cur = 0, sp = 0;
    for (;;) {
      const float4 *N = nodes + (size_t)cur * 8;
      const float4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3], q4 = N[4], q5 = N[5], q6 = N[6];
      float b0 = np_box_bound(q0.x, q1.x, q2.x, q3.x, q4.x, q5.x, p.x, p.y, p.z, mw);
      float b1 = np_box_bound(q0.y, q1.y, q2.y, q3.y, q4.y, q5.y, p.x, p.y, p.z, mw);
      float b2 = np_box_bound(q0.z, q1.z, q2.z, q3.z, q4.z, q5.z, p.x, p.y, p.z, mw);
      float b3 = np_box_bound(q0.w, q1.w, q2.w, q3.w, q4.w, q5.w, p.x, p.y, p.z, mw);
      uint32_t c0 = bits(q6.x), c1 = bits(q6.y), c2 = bits(q6.z), c3 = bits(q6.w);
      // ascending bounds: the five compare-exchanges that sort four
#define NP_CSWAP(bi, ci, bj, cj)                 \
  {                                              \
    const bool s = bj < bi;                      \
    const float tb = s ? bj : bi;                \
    const uint32_t tc = s ? cj : ci;             \
    bj = s ? bi : bj;                            \
    cj = s ? ci : cj;                            \
    bi = tb;                                     \
    ci = tc;                                     \
  }
      NP_CSWAP(b0, c0, b1, c1) NP_CSWAP(b2, c2, b3, c3) NP_CSWAP(b0, c0, b2, c2) NP_CSWAP(b1, c1, b3, c3) NP_CSWAP(b1, c1, b2, c2)
#undef NP_CSWAP
#define NP_LEAF(b, c)                                                                \
  if ((c & BVH_LEAF_FLAG) && !(b > md2)) {                                           \
    const uint32_t first = tri_begin + (c & 0xFFFFFFu), n = (c >> 24) & 0x7Fu;       \
    for (uint32_t j = 0; j < n; ++j) test(first + j);                                \
  }
      NP_LEAF(b0, c0) NP_LEAF(b1, c1) NP_LEAF(b2, c2) NP_LEAF(b3, c3)
#undef NP_LEAF
      uint32_t next = RQ_NONE;
#define NP_INNER(b, c)                                                   \
  if (!(c & BVH_LEAF_FLAG) && !(b > md2)) {                              \
    if (next != RQ_NONE && sp < S.slots) stk[(sp++) * STRIDE] = next;    \
    next = c;                                                            \
  }
      NP_INNER(b3, c3) NP_INNER(b2, c2) NP_INNER(b1, c1) NP_INNER(b0, c0)
#undef NP_INNER
      if (next == RQ_NONE) {
        if (sp == 0) break;
        next = stk[(--sp) * STRIDE];
      }
      cur = next;
    }
  }
  if (morig != RQ_NONE && best.beaten_by(md2, index)) {
    best.d2 = md2;
    best.obj = index;
    best.rec = mrec;
    best.gn = tri_begin + morig;
    best.prim = morig;
  }
}

// V: RQ_LINEAR or 0
template <uint32_t V>
__global__ __launch_bounds__(RQ_THREADS) void ray_nearest_kernel(NearestLaunch L) {
  extern __shared__ uint32_t rq_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RQ_THREADS + threadIdx.x;
  if (i >= L.n_points) return;
  const Scene S = make_scene(L.scene, 0u);
  uint32_t *stk = rq_stack + threadIdx.x;
  const size_t i3 = (size_t)i * 3;
  const V3 p = mk(L.point[i3], L.point[i3 + 1], L.point[i3 + 2]);
  const float md = L.max_dist_arr ? L.max_dist_arr[i] : L.max_dist;
  const uint32_t only = (uint32_t)L.only;  // RQ_NONE: every object
  Near best;
  best.d2 = md * md;
  // a point that is not finite has no finite d2 with anything, a limit that is NaN or negative admits nothing: the miss values
  const bool live = md >= 0.0f && fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
  if (live) {
    // ---- planes (two per record, coordinates interleaved) ----
    if (!(L.flags & CTR_NEAREST_SKIP_PLANES)) {
      for (uint32_t r = 0; r < S.n_plane_recs; ++r) {
        const float4 *P = S.planes + (size_t)r * 4;
        const float4 w0 = P[0], w1 = P[1], w2 = P[2], w3 = P[3];
        const float px[2] = {w0.x, w0.y}, py[2] = {w0.z, w0.w}, pz[2] = {w1.x, w1.y};
        const float nx[2] = {w1.z, w1.w}, ny[2] = {w2.x, w2.y}, nz[2] = {w2.z, w2.w};
        const uint32_t idx[2] = {bits(w3.x), bits(w3.y)};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (idx[s] == CTR_PLANE_PAD || (only != RQ_NONE && idx[s] != only)) continue;
          const NpCand c = np_plane(px[s], py[s], pz[s], nx[s], ny[s], nz[s], p.x, p.y, p.z);
          if (best.beaten_by(c.d2, idx[s])) {
            best.d2 = c.d2;
            best.obj = idx[s];
          }
        }
      }
    }
    // ---- spheres and stand-alone triangles, scene order ----
    for (uint32_t k = 0; k < S.n_oloop; ++k) {
      const float4 *O = S.oloop + (size_t)k * 4;
      const float4 o0 = O[0], o1 = O[1], o2 = O[2];
      const uint32_t index = bits(o1.w);
      if (only != RQ_NONE && index != only) continue;
      NpCand c;
      uint32_t rec = RQ_NONE;
      if (bits(o0.x) == CTR_OBJ_SPHERE) {
        c = np_sphere(o2.x, o2.y, o2.z, o2.w, p.x, p.y, p.z);
      } else {
        uint32_t unused;
        rec = bits(o0.z);
        c = tri_cand(S.tris + (size_t)rec * 4, p, unused);
      }
      if (best.beaten_by(c.d2, index)) {
        best.d2 = c.d2;
        best.obj = index;
        best.rec = rec;
        best.gn = rec;
        best.prim = RQ_NONE;
      }
    }
    // ---- meshes ----
    for (uint32_t m = 0; m < S.n_mesh; ++m) {
      const float4 *O = S.meshes + (size_t)m * 4;
      if (only != RQ_NONE && bits(O[1].w) != only) continue;
      nearest_mesh<(V & RQ_LINEAR) != 0>(S, O, p, best, stk);
    }
  }
  // ---- the answer: the winner's candidate once more (the same operations, the same bits), and its normal ----
  float dist = INFINITY;
  V3 q = mk(0, 0, 0), nrm = mk(0, 0, 0);
  if (best.obj != RQ_NONE) {
    const float4 *H = S.objs + (size_t)best.obj * 4;
    const float4 h0 = H[0], h2 = H[2], h3 = H[3];
    const uint32_t type = bits(h0.x);
    NpCand c;
    if (type == CTR_OBJ_SPHERE) {
      c = np_sphere(h2.x, h2.y, h2.z, h2.w, p.x, p.y, p.z);
      nrm = vnormalized(vsub(mk(c.qx, c.qy, c.qz), mk(h2.x, h2.y, h2.z)));
    } else if (type == CTR_OBJ_PLANE) {
      c = np_plane(h2.x, h2.y, h2.z, h2.w, h3.x, h3.y, p.x, p.y, p.z);
      nrm = mk(h2.w, h3.x, h3.y);
    } else {
      uint32_t unused;
      c = tri_cand(S.tris + (size_t)best.rec * 4, p, unused);
      const float *g = S.gnorm + (size_t)best.gn * 4;
      nrm = mk(g[0], g[1], g[2]);
    }
    dist = sqrtf(best.d2);
    q = mk(c.qx, c.qy, c.qz);
  }
  if (L.distance) L.distance[i] = dist;
  if (L.object) L.object[i] = (int32_t)best.obj;
  if (L.prim) L.prim[i] = best.prim != RQ_NONE ? (int32_t)best.prim : -1;
  if (L.nearest) { L.nearest[i3] = q.x; L.nearest[i3 + 1] = q.y; L.nearest[i3 + 2] = q.z; }
  if (L.normal) { L.normal[i3] = nrm.x; L.normal[i3 + 1] = nrm.y; L.normal[i3 + 2] = nrm.z; }
}

}  // namespace

int ctr_launch_nearest(const NearestLaunch &L, void *stream) {
  if (L.n_points == 0) return 0;
  const bool lin = (L.flags & CTR_NEAREST_LINEAR) != 0;
  void (*kernel)(NearestLaunch) = lin ? ray_nearest_kernel<RQ_LINEAR> : ray_nearest_kernel<0u>;
  return launch_lanes(kernel, L, L.n_points, RQ_THREADS, walk_stack_bytes(L.scene.stack_slots, RQ_THREADS, lin), (hipStream_t)stream);
}
