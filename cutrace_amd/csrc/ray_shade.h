// ray_shade.h — what ctr_shade_rays (ctr_rays.cpp) hands the radiance-query kernel (ray_shade.hip).
#ifndef CUTRACE_AMD_RAY_SHADE_H
#define CUTRACE_AMD_RAY_SHADE_H

#include <stddef.h>
#include <stdint.h>

#include "ray_query.h"
#include "scene_device.h"

struct ShadeLaunch {
  RayScene scene;           // (ray_query.h)
  const DLight *lights;
  uint32_t n_light;
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
