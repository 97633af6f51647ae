// ray_query.hip — the kernel behind ctr_cast_rays (include/cutrace_rays.h): rays from memory, not from a camera.
//
// What it restates (reference, file:line), with the render kernel's numerics (render_kernel.hip, "Numerics"):
//   ray_cast            inc/ray_cast.hpp:29-55      nearest hit over every object, ties to the lower object index
//   shadow_intensity    inc/shading.hpp:22-45       CTR_RAY_SHADOW: a loop of nearest casts, 1 - transparency per hit
//   triangle / mesh / plane / sphere::intersect, uv_for   inc/default_schema.hpp:37-251
//
// The render kernel casts an 8x8 pixel tile per wave: its rays are coherent, so the whole wave walks ONE path through
// the scene (the union of its lanes' nodes) with every record in SGPRs.  A caller's rays come in any order, and that
// trade turns: here ONE LANE = ONE RAY, each lane walking its own.  Records arrive through vector loads (16-byte
// aligned: every record is 64 or 128 bytes, every array a hipMalloc), each mesh's four-wide BVH (bvh.h) is walked with
// a per-lane stack in LDS laid out [entry][lane] (conflict-free whatever depth each lane is at), sized from the
// scene's deepest mesh tree (scene_flatten.h FlatScene::ray_slots).  No scratch memory.  The walk itself (cast, cast_mesh,
// tri_hit) lives in ray_walk.h, which the radiance queries (ray_shade.hip) share; the hit record in hit_record.h, which the hit lists (ray_hits.hip) share.
//
// Exactness — what each step may and may not shortcut:
//  * planes, spheres, stand-alone triangles: the reference's arithmetic, operation for operation (-ffp-contract=off,
//    IEEE division and square root);
//  * a mesh: first the reference's AABB test (bound_intersects: IEEE reciprocals, tmin from 0, std::min/max selects);
//    then its triangles in order (CTR_RAY_LINEAR), or its BVH.  The BVH's box test is the render kernel's: a world-space
//    margin of 2^-14 x the distance from the origin to the mesh box, 1-ulp reciprocals clamped to +-1e30 (of the direction
//    scaled by a power of two to unit size, so that a direction of any length gets that direction's test), the same FMAs,
//    a NaN dropping its axis' constraint; a child is entered unless max(entry, min_t) > min(exit, limit) — so a box
//    that only ties the nearest hit so far is still entered.  Culling is exact except for rays in a triangle's plane
//    (the header says which); LINEAR is exact for every ray;
//  * a triangle: the reference's four determinants in its order; the three IEEE divisions are skipped only where a
//    1-ulp reciprocal decides the five comparisons for certain (the render kernel's margins), and t0 is divided exactly
//    wherever its value can still matter (it can beat or tie the nearest hit);
//  * CTR_RAY_SHADOW on a scene whose materials are all opaque: the loop's first cast decides (intensity 0 or 1), and it
//    stops at the first object whose accepted t lies below max_t.  A mesh counts only with its NEAREST valid t (a mesh
//    whose nearest valid t equals min_t is rejected whole), so a mesh is always walked to its end.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "cutrace_rays.h"
#include "hit_record.h"
#include "ray_launch.h"
#include "ray_query.h"
#include "ray_walk.h"
#include "scene_device.h"

namespace {

template <uint32_t V>
__global__ __launch_bounds__(RQ_THREADS) void ray_query_kernel(RayLaunch L) {
  extern __shared__ uint32_t rq_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RQ_THREADS + threadIdx.x;
  if (i >= L.n_rays) return;
  const Scene S = make_scene(L.scene, L.flags & CTR_RAY_IGNORE_TRANSPARENT);
  uint32_t *stk = rq_stack + threadIdx.x;
  const size_t i3 = (size_t)i * 3;
  const V3 ro = mk(L.origin[i3], L.origin[i3 + 1], L.origin[i3 + 2]);
  const V3 rd = mk(L.dir[i3], L.dir[i3 + 1], L.dir[i3 + 2]);
  if (V & RQ_SHADOW) {
    // ---- shadow_intensity, shading.hpp:22-45 ----
    const float max_t = L.max_t_arr ? L.max_t_arr[i] : L.max_t;
    float intensity = 0.0f, last_hit = 0.0f;
    for (;;) {
      // shading.hpp:32: `last_hit + 1e-3` is a DOUBLE add narrowed to float at the call
      const Best h = cast<V>(S, ro, rd, (float)((double)last_hit + 1e-3), max_t, stk);
      if (!(h.obj != RQ_NONE && h.t < max_t)) break;
      if (V & RQ_ANYHIT) {  // every material opaque: 1 - transparency is 1
        intensity = 1.0f;
        break;
      }
      const uint32_t mat = bits(S.objs[(size_t)h.obj * 4].y);
      intensity += (1.0f - L.scene.mats[mat].transparency);  // get_bounce_params, default_schema.hpp:337-340
      if (intensity >= 1.0f) {
        intensity = 1.0f;
        break;
      }
      last_hit = h.t;
    }
    L.shadow[i] = intensity;
    return;
  }
  const float min_t = L.min_t_arr ? L.min_t_arr[i] : L.min_t;
  const Best b = cast<V>(S, ro, rd, min_t, INFINITY, stk);
  const bool hit = b.obj != RQ_NONE;
  if (L.t) L.t[i] = b.t;
  if (L.object) L.object[i] = hit ? (int32_t)b.obj : -1;
  if (L.prim) L.prim[i] = (hit && b.prim != RQ_NONE) ? (int32_t)b.prim : -1;
  if (!(L.point || L.normal || L.uv)) return;
  // ---- the hit record: point, normal (per primitive), texture coordinates (hit_record.h) ----
  const HitRecord r = hit_record(S, ro, rd, b);
  const V3 pos = r.pos, nrm = r.nrm;
  const float u = r.u, v = r.v;
  if (L.point) { L.point[i3] = pos.x; L.point[i3 + 1] = pos.y; L.point[i3 + 2] = pos.z; }
  if (L.normal) { L.normal[i3] = nrm.x; L.normal[i3 + 1] = nrm.y; L.normal[i3 + 2] = nrm.z; }
  if (L.uv) { L.uv[2 * (size_t)i] = u; L.uv[2 * (size_t)i + 1] = v; }
}

}  // namespace

int ctr_launch_rays(const RayLaunch &L, void *stream) {
  if (L.n_rays == 0) return 0;
  const bool lin = (L.flags & CTR_RAY_LINEAR) != 0;
  void (*kernel)(RayLaunch);
  if (!(L.flags & CTR_RAY_SHADOW)) kernel = lin ? ray_query_kernel<RQ_LINEAR> : ray_query_kernel<0u>;
  else if (L.anyhit) kernel = lin ? ray_query_kernel<RQ_SHADOW | RQ_ANYHIT | RQ_LINEAR> : ray_query_kernel<RQ_SHADOW | RQ_ANYHIT>;
  else kernel = lin ? ray_query_kernel<RQ_SHADOW | RQ_LINEAR> : ray_query_kernel<RQ_SHADOW>;
  return launch_lanes(kernel, L, L.n_rays, RQ_THREADS, walk_stack_bytes(L.scene.stack_slots, RQ_THREADS, lin), (hipStream_t)stream);
}
