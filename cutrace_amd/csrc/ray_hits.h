// ray_hits.h — what ctr_list_hits (ctr_rays.cpp) hands the hit-list kernel (ray_hits.hip).
#ifndef CUTRACE_AMD_RAY_HITS_H
#define CUTRACE_AMD_RAY_HITS_H

#include <stdint.h>

#include "ray_query.h"

struct HitsLaunch {
  RayScene scene;
  // the query (include/cutrace_hits.h)
  uint32_t n_rays, flags, max_hits;
  float min_t, max_t;
  double step;
  const float *origin, *dir, *min_t_arr, *max_t_arr;
  int32_t *count;
  // per-slot outputs, slot-major: slot j of ray i at element j * n_rays + i
  float *t, *point, *normal, *uv;
  int32_t *object, *prim;
};

// host-callable launcher implemented in ray_hits.hip; returns a hipError_t as int
int ctr_launch_hits(const HitsLaunch &L, void *stream);

#endif
