/*
 * cutrace_rays.h — cast caller-supplied rays against a scene uploaded with ctr_scene_create.
 *
 * One entry point, ctr_cast_rays, answers per ray what the reference answers for its own rays:
 *
 *   nearest-hit mode (default)  ray_cast(scene, ray, min_t, ..., ignore_transparent)   inc/ray_cast.hpp:29-55
 *   CTR_RAY_SHADOW              shadow_intensity(scene, ray, max_t)                     inc/shading.hpp:22-45
 *
 * with the render kernel's numerics: every object in scene order, ties on t to the lower object index (inside a mesh
 * to the lower file index), a mesh whose nearest valid t equals min_t rejected whole, the mesh's AABB test first.
 * The results are bit-identical to the reference compiled for the host, except the sphere's texture coordinates
 * (atan2f / asinf, within 1e-4).  A sphere normalises the direction: its t and hit point are measured along dir /
 * |dir|, every other object's along dir itself (the reference's own unit mix; directions need not be normalised).
 *
 * Exactness of the default walk: each mesh is walked through its BVH, whose culling is exact except for a ray that
 * lies IN a triangle's plane to within rounding (origin in the plane, direction parallel to it); there the
 * reference's float test can accept a triangle the ray passes far from.  Eyes, lights and mirror images of the
 * scene's cameras are guarded; arbitrary query origins are not.  CTR_RAY_LINEAR walks every
 * mesh's triangles linearly after the AABB test and is bit-identical to the reference for every ray.
 *
 * Calls are asynchronous on `hip_stream`, allocate nothing and never synchronise (a call can be captured into a
 * graph), and use no per-handle scratch (later renders and their counters are undisturbed).  Like renders, calls on
 * one handle must be ordered by the caller against ctr_scene_set_cameras and ctr_set_variant(CTR_VAR_MERGE), which
 * rewrite device arrays.
 */
#ifndef CUTRACE_RAYS_H
#define CUTRACE_RAYS_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_RAY_IGNORE_TRANSPARENT 1u /* ray_cast's ignore_transparent = true: objects whose material has
                                        transparency >= 1e-6 (a double comparison) do not exist for the cast */
#define CTR_RAY_LINEAR 2u             /* walk meshes linearly: exact also for rays in a triangle's plane        */
#define CTR_RAY_SHADOW 4u             /* shadow_intensity instead of ray_cast                                  */

typedef struct ctr_ray_query {
  uint64_t n_rays;         /* < 2^31; 0: nothing is launched                                                      */
  uint32_t flags;          /* CTR_RAY_*                                                                           */
  float min_t;             /* nearest-hit: every ray's min_dist when d_min_t is NULL (SHADOW: unused, the loop
                              starts at (float)(0.0 + 1e-3) as the reference's does)                             */
  float max_t;             /* SHADOW: every ray's max_dist when d_max_t is NULL                                   */
  uint32_t reserved;       /* 0                                                                                   */
  const float *d_origin;   /* n x 3, device memory of the scene's device (as every pointer below)                */
  const float *d_dir;      /* n x 3                                                                               */
  const float *d_min_t;    /* optional: n per-ray min_dist values (nearest-hit)                                   */
  const float *d_max_t;    /* optional: n per-ray max_dist values (SHADOW)                                        */
  /* nearest-hit outputs, each optional (NULL = not written), at least one required:                              */
  float *d_t;              /* n: distance, +inf on a miss                                                         */
  int32_t *d_object;       /* n: index into ctr_scene_desc.objects, -1 on a miss                                  */
  int32_t *d_prim;         /* n: a mesh hit's triangle, file order within the mesh; -1 otherwise                  */
  float *d_point;          /* n x 3: hit point (0, 0, 0 on a miss)                                                */
  float *d_normal;         /* n x 3: the reference's normal (0, 0, 0 on a miss)                                   */
  float *d_uv;             /* n x 2: texture coordinates as ctr_render_uv gives them (0, 0 on a miss)             */
  /* SHADOW output, required there and only there:                                                              */
  float *d_shadow;         /* n: intensity in [0, 1], 1 = fully blocked                                           */
} ctr_ray_query;

/* Casts q->n_rays rays on `hip_stream` (NULL: the null stream of the scene's device).  CTR_E_INVALID, with a
 * ctr_last_error message, for: a NULL scene or query; NULL rays when n_rays > 0; unknown flag bits; SHADOW together
 * with IGNORE_TRANSPARENT; SHADOW with a nearest-hit output or without d_shadow; nearest-hit mode without any output
 * or with d_shadow; a pointer that is not device memory of the scene's device; n_rays >= 2^31. */
int ctr_cast_rays(ctr_scene *scene, const ctr_ray_query *q, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
