// ray_points.h — what ctr_shade_points (ctr_rays.cpp) hands the surface-shading kernel (ray_points.hip).
#ifndef CUTRACE_AMD_RAY_POINTS_H
#define CUTRACE_AMD_RAY_POINTS_H

#include <stddef.h>
#include <stdint.h>

#include "ray_query.h"
#include "scene_device.h"

struct PointsLaunch {
  RayScene scene;           // (ray_query.h)
  const DLight *lights;
  uint32_t n_light;
  uint32_t n_mat, n_obj;     // what a per-point material / object index is checked against
  uint32_t all_opaque;       // no material transmits: a shadow cast stops at the first occluder
  // the query (include/cutrace_rays.h)
  uint32_t n_points, flags;  // flags: CTR_POINTS_*, EXACT_POW also set for a scene outside the fast path's domain
  int32_t material;          // every point's material when both arrays below are null
  float ambient;
  const float *point, *normal, *view;
  const int32_t *mat_arr, *obj_arr;
  float *color, *light_shadow;
};

// lanes per workgroup, and the dynamic LDS of one workgroup of the launch in bytes (the walk's stack; none when linear)
#define CTR_POINTS_THREADS 128
#define CTR_POINTS_LDS_MAX 65536u
size_t ctr_points_lds_bytes(const PointsLaunch &L);

// host-callable launcher implemented in ray_points.hip; returns a hipError_t as int
int ctr_launch_points(const PointsLaunch &L, void *stream);

#endif
