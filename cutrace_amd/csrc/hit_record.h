// hit_record.h — what ray_cast returns besides t and the object (ray_cast.hpp:44-47): the hit point, the normal of the
// primitive that was hit, and the texture coordinates of the hit, for one ray's nearest hit `b` (ray_walk.h Best).
//
// One text for ray_query.hip (ctr_cast_rays) and ray_hits.hip (ctr_list_hits).  Device code only, after ray_walk.h's includes.
#ifndef CUTRACE_AMD_HIT_RECORD_H
#define CUTRACE_AMD_HIT_RECORD_H

#include "ray_walk.h"

namespace {

struct HitRecord {
  V3 pos, nrm;
  float u, v;
};

// a miss: zeros (uv{} of kernel.hpp:51)
__device__ __forceinline__ HitRecord hit_record(const Scene &S, V3 ro, V3 rd, const Best &b) {
  V3 pos = mk(0, 0, 0), nrm = mk(0, 0, 0);
  float u = 0.0f, v = 0.0f;
  if (b.obj != RQ_NONE) {
    const float4 *H = S.objs + (size_t)b.obj * 4;
    const float4 h0 = H[0], h2 = H[2], h3 = H[3];
    const uint32_t type = bits(h0.x);
    if (type == CTR_OBJ_SPHERE) {
      // default_schema.hpp:245-249: the hit uses the NORMALISED direction; uv's delta is the normal again
      pos = vadd(ro, vscale(vnormalized(rd), b.t));
      nrm = vnormalized(vsub(pos, mk(h2.x, h2.y, h2.z)));
      u = 0.5f + (atan2f(nrm.z, nrm.x) / (2.0f * (float)M_PI));
      v = 0.5f + (asinf(nrm.y) / (float)M_PI);
    } else {
      pos = vadd(ro, vscale(rd, b.t));  // start + dist*dir
      if (type == CTR_OBJ_PLANE) {
        nrm = mk(h2.w, h3.x, h3.y);
        // plane::uv_for, default_schema.hpp:169-178
        const V3 ax1 = vnormalized(mk(nrm.y, -nrm.x, 0.0f));
        const V3 ax2 = vcross(nrm, ax1);
        const V3 mod_pt = vsub(mk(h2.x, h2.y, h2.z), pos);
        u = vdot(ax1, mod_pt);
        v = vdot(ax2, mod_pt);
      } else {
        const float *g = S.gnorm + (size_t)b.tri * 4;
        nrm = mk(g[0], g[1], g[2]);
        if (type == CTR_OBJ_MESH) {  // mesh::intersect, default_schema.hpp:138-139
          u = pos.x;
          v = pos.y;
        } else {  // triangle::uv_for, default_schema.hpp:37-46 (p1, p3 in the object record, p2 in its DTri)
          const float4 *T = S.tris + (size_t)b.tri * 4;
          const float4 t1 = T[1], t2 = T[2];
          const V3 p1 = mk(h2.x, h2.y, h2.z), p2 = mk(t1.z, t1.w, t2.x), p3 = mk(h2.w, h3.x, h3.y);
          const V3 p2p1 = vsub(p2, p1), p3p1 = vsub(p3, p1), xp1 = vsub(pos, p1);
          const V3 proj_u = vscale(p2p1, vdot(xp1, p2p1) / vdot(p2p1, p2p1));
          const V3 proj_v = vscale(p3p1, vdot(xp1, p3p1) / vdot(p3p1, p3p1));
          u = vnorm(proj_u) / vnorm(p2p1);
          v = vnorm(proj_v) / vnorm(p3p1);
        }
      }
    }
  }
  HitRecord r;
  r.pos = pos;
  r.nrm = nrm;
  r.u = u;
  r.v = v;
  return r;
}

}  // namespace

#endif
