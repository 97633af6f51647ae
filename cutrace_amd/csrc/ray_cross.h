// ray_cross.h — what ctr_count_crossings and ctr_inside_points (ctr_rays.cpp) hand the kernels of ray_cross.hip.
#ifndef CUTRACE_AMD_RAY_CROSS_H
#define CUTRACE_AMD_RAY_CROSS_H

#include <stdint.h>

#include "ray_query.h"

constexpr uint32_t CROSS_MAX_DIRS = 15;  // CTR_INSIDE_MAX_DIRS

// the default directions of ctr_inside_points (include/cutrace_inside.h), x y z each
constexpr float CROSS_DEFAULT_DIRS[9] = {0.3713907f, 0.5570860f, 0.7427814f, -0.6396021f, 0.7462025f, -0.1842720f,
                                         0.8017837f, -0.2672612f, -0.5345225f};

struct CrossLaunch {
  RayScene scene;
  // the query (include/cutrace_inside.h)
  uint32_t n_rays, flags;
  int32_t only;  // -1: every object; else the one object counted
  float min_t, max_t;
  const float *origin, *dir, *min_t_arr, *max_t_arr;
  int32_t *count, *sgn;
};

struct InsideLaunch {
  RayScene scene;
  uint32_t n_points, flags;
  int32_t only;     // -1: every mesh and sphere; else the one mesh or sphere counted
  uint32_t n_dirs;  // R: odd, 1 .. CROSS_MAX_DIRS
  float dirs[CROSS_MAX_DIRS * 3];  // the same for every lane: scalar data of the kernel
  const float *point;
  uint8_t *inside, *votes;
  float *distance;  // in and out: negated where the point is inside
};

// host-callable launchers implemented in ray_cross.hip; each returns a hipError_t as int
int ctr_launch_cross(const CrossLaunch &L, void *stream);
int ctr_launch_inside(const InsideLaunch &L, void *stream);

#endif
