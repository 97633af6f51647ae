// ray_hits.hip — the kernel behind ctr_list_hits (include/cutrace_hits.h): the first K hits along each ray.
//
// What it restates (reference, file:line): the chain of nearest casts inside shadow_intensity, inc/shading.hpp:22-45 —
// each cast (ray_cast, inc/ray_cast.hpp:29-55) starts at (float)((double)last_hit + step), shading.hpp:32, and the chain
// ends at the first cast that hits nothing below max_t, shading.hpp:33 — without the sum: the hits themselves.
//
// ONE LANE = ONE RAY, as in ray_query.hip, whose walk (ray_walk.h cast<V>, the per-lane LDS stack laid out [entry][lane])
// and whose hit record (hit_record.h) this kernel shares: each cast of a chain is ctr_cast_rays' cast, operation for
// operation.  The lane reads its ray once and keeps it, and the scene head, in registers across the chain.  It stores slot
// j inside the loop — the outputs are SLOT-MAJOR (slot j of ray i at j * n + i), so neighbouring lanes write neighbouring
// addresses — and never holds more than one hit record.  After the loop it writes ctr_cast_rays' miss values into its
// remaining slots, then the count.  Every cast is limited to max_t, as the shadow loop's are: nothing beyond it is listed.
//
// A wave runs as long as its longest chain; lanes whose chain has ended idle meanwhile.  Accepted: the alternative, a
// launch per layer (what a loop of ctr_cast_rays does), reloads every ray and the scene head per layer and runs every
// layer at the batch's full width.  No scratch memory; LDS is the ray query's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "cutrace_hits.h"
#include "hit_record.h"
#include "ray_hits.h"
#include "ray_launch.h"
#include "ray_walk.h"
#include "scene_device.h"

namespace {

template <uint32_t V>
__global__ __launch_bounds__(RQ_THREADS) void ray_hits_kernel(HitsLaunch L) {
  extern __shared__ uint32_t rq_stack[];
  const uint32_t i = blockIdx.x * (uint32_t)RQ_THREADS + threadIdx.x;
  if (i >= L.n_rays) return;
  const Scene S = make_scene(L.scene, L.flags & CTR_HITS_IGNORE_TRANSPARENT);
  uint32_t *stk = rq_stack + threadIdx.x;
  const size_t i3 = (size_t)i * 3;
  const V3 ro = mk(L.origin[i3], L.origin[i3 + 1], L.origin[i3 + 2]);
  const V3 rd = mk(L.dir[i3], L.dir[i3 + 1], L.dir[i3 + 2]);
  const float max_t = L.max_t_arr ? L.max_t_arr[i] : L.max_t;
  const bool slots = L.t || L.object || L.prim || L.point || L.normal || L.uv;
  const bool records = L.point || L.normal || L.uv;
  float m = L.min_t_arr ? L.min_t_arr[i] : L.min_t;
  size_t at = i;  // slot j of this ray: element j * n_rays + i (below 2^31 whenever a slot output exists)
  uint32_t j = 0;
  for (; j < L.max_hits; ++j, at += L.n_rays) {
    const Best h = cast<V>(S, ro, rd, m, max_t, stk);
    if (!(h.obj != RQ_NONE && h.t < max_t)) break;  // shading.hpp:33
    if (L.t) L.t[at] = h.t;
    if (L.object) L.object[at] = (int32_t)h.obj;
    if (L.prim) L.prim[at] = h.prim != RQ_NONE ? (int32_t)h.prim : -1;
    if (records) {
      const HitRecord r = hit_record(S, ro, rd, h);
      if (L.point) { L.point[at * 3] = r.pos.x; L.point[at * 3 + 1] = r.pos.y; L.point[at * 3 + 2] = r.pos.z; }
      if (L.normal) { L.normal[at * 3] = r.nrm.x; L.normal[at * 3 + 1] = r.nrm.y; L.normal[at * 3 + 2] = r.nrm.z; }
      if (L.uv) { L.uv[at * 2] = r.u; L.uv[at * 2 + 1] = r.v; }
    }
    m = (float)((double)h.t + L.step);  // shading.hpp:32: a DOUBLE add narrowed to float at the call
  }
  // the slots the chain did not reach: what ctr_cast_rays writes on a miss (a query for the count alone has none to fill)
  for (uint32_t k = j; slots && k < L.max_hits; ++k, at += L.n_rays) {
    if (L.t) L.t[at] = INFINITY;
    if (L.object) L.object[at] = -1;
    if (L.prim) L.prim[at] = -1;
    if (L.point) { L.point[at * 3] = 0.0f; L.point[at * 3 + 1] = 0.0f; L.point[at * 3 + 2] = 0.0f; }
    if (L.normal) { L.normal[at * 3] = 0.0f; L.normal[at * 3 + 1] = 0.0f; L.normal[at * 3 + 2] = 0.0f; }
    if (L.uv) { L.uv[at * 2] = 0.0f; L.uv[at * 2 + 1] = 0.0f; }
  }
  if (L.count) L.count[i] = (int32_t)j;
}

}  // namespace

int ctr_launch_hits(const HitsLaunch &L, void *stream) {
  if (L.n_rays == 0) return 0;
  const bool lin = (L.flags & CTR_HITS_LINEAR) != 0;
  void (*kernel)(HitsLaunch) = lin ? ray_hits_kernel<RQ_LINEAR> : ray_hits_kernel<0u>;
  return launch_lanes(kernel, L, L.n_rays, RQ_THREADS, walk_stack_bytes(L.scene.stack_slots, RQ_THREADS, lin), (hipStream_t)stream);
}
