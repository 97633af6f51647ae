// ray_shade.h — what ctr_shade_rays (ctr_api.cpp) hands the radiance-query kernel (ray_shade.hip).
#ifndef CUTRACE_AMD_RAY_SHADE_H
#define CUTRACE_AMD_RAY_SHADE_H

#include <stddef.h>
#include <stdint.h>

#include "scene_device.h"

struct ShadeLaunch {
  // the scene's device arrays, as the render kernel reads them (scene_device.h, bvh.h)
  const DObj *objs;          // every object, scene order (hit records)
  const DObj *oloop;         // spheres and stand-alone triangles, scene order
  const DObj *meshes;        // non-empty meshes (the first n_mesh records: the regular ones, never the merged tree)
  const DPlanePair *planes;
  const DTri *tris;
  const void *nodes4;        // DNode4[]: per-mesh trees
  const float *gnorm;
  const DMat *mats;
  const DLight *lights;
  uint32_t n_oloop, n_plane_recs, n_mesh, n_light;
  uint32_t stack_slots;      // LDS walk-stack entries per lane (scene_flatten.h FlatScene::ray_slots)
  uint32_t frames;           // LDS recursion frames per lane (ctr_shade_frames)
  uint32_t frame_dwords;     // 4, or 10 when some material both reflects and transmits (FlatScene::need_cold)
  uint32_t all_opaque;       // no material transmits: a shadow cast stops at the first occluder
  // the query (include/cutrace_rays.h)
  uint32_t n_rays, flags;
  int32_t bounces;
  float min_t, ambient;
  const float *origin, *dir;
  float *color, *t, *normal;
  int32_t *object;
};

// recursion frames a lane can push: one per level below the first, none when nothing reflects or transmits
inline uint32_t ctr_shade_frames(int bounces, bool any_bounce) { return any_bounce && bounces > 0 ? (uint32_t)bounces : 0u; }
// dynamic LDS of one workgroup of the launch, in bytes (ray_shade.hip); what one workgroup may ask for at most
size_t ctr_shade_lds_bytes(const ShadeLaunch &L);
#define CTR_SHADE_LDS_MAX 65536u

// host-callable launcher implemented in ray_shade.hip; returns a hipError_t as int
int ctr_launch_shade(const ShadeLaunch &L, void *stream);

#endif
