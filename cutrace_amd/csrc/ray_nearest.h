// ray_nearest.h — what ctr_nearest_points (ctr_rays.cpp) hands the nearest-point kernel (ray_nearest.hip).
#ifndef CUTRACE_AMD_RAY_NEAREST_H
#define CUTRACE_AMD_RAY_NEAREST_H

#include <stdint.h>

#include "ray_query.h"

struct NearestLaunch {
  RayScene scene;
  // the query (include/cutrace_nearest.h)
  uint32_t n_points, flags;
  int32_t only;  // -1: every object; else the one object admitted
  float max_dist;
  const float *point, *max_dist_arr;
  float *distance, *nearest, *normal;
  int32_t *object, *prim;
};

// host-callable launcher implemented in ray_nearest.hip; returns a hipError_t as int
int ctr_launch_nearest(const NearestLaunch &L, void *stream);

#endif
