// ray_query.h — what ctr_cast_rays (ctr_rays.cpp) hands the ray-query kernel (ray_query.hip), and the description of the
// scene (RayScene) that it shares with the radiance queries (ray_shade.h).
#ifndef CUTRACE_AMD_RAY_QUERY_H
#define CUTRACE_AMD_RAY_QUERY_H

#include <stddef.h>
#include <stdint.h>

#include "scene_device.h"

// the scene's device arrays, as the render kernel reads them (scene_device.h, bvh.h): what the walk of ray_walk.h needs
struct RayScene {
  const DObj *objs;          // every object, scene order (hit records)
  const DObj *oloop;         // spheres and stand-alone triangles, scene order
  const DObj *meshes;        // non-empty meshes (the first n_mesh records: the regular ones, never the merged tree)
  const DPlanePair *planes;
  const DTri *tris;
  const void *nodes4;        // DNode4[]: per-mesh trees
  const float *gnorm;
  const DMat *mats;
  uint32_t n_oloop, n_plane_recs, n_mesh;
  uint32_t stack_slots;      // LDS stack entries per lane the deepest mesh tree needs (scene_flatten.h FlatScene::ray_slots)
};

// dynamic LDS of the walk's stack for one workgroup of `lanes` lanes, in bytes: [entry][lane] dwords, none for a linear walk
constexpr size_t walk_stack_bytes(uint32_t slots, uint32_t lanes, bool linear) {
  return linear ? 0 : (size_t)slots * lanes * sizeof(uint32_t);
}

struct RayLaunch {
  RayScene scene;
  // the query (include/cutrace_rays.h)
  uint32_t n_rays, flags;
  bool anyhit;               // SHADOW on a scene whose materials are all opaque: stop at the first occluder
  float min_t, max_t;
  const float *origin, *dir, *min_t_arr, *max_t_arr;
  float *t, *point, *normal, *uv, *shadow;
  int32_t *object, *prim;
};

// host-callable launcher implemented in ray_query.hip; returns a hipError_t as int
int ctr_launch_rays(const RayLaunch &L, void *stream);

#endif
