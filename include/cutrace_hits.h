/*
 * cutrace_hits.h — hit lists: the first K hits along each caller-supplied ray, against a scene uploaded with
 * ctr_scene_create.
 *
 * ctr_cast_rays (cutrace_rays.h) answers the nearest hit, and its CTR_RAY_SHADOW mode one number for everything between
 * a point and a light.  ctr_list_hits answers what lies behind the first hit: the chain of nearest casts that the
 * reference's shadow_intensity walks (inc/shading.hpp:22-45; the restart of each cast is shading.hpp:32), itself, one
 * lane per ray, in one launch.  For ray i, with K = max_hits:
 *
 *   m = min_t_i
 *   for j = 0 .. K-1:
 *       h = ray_cast(scene, ray, m, ignore_transparent)                                 inc/ray_cast.hpp:29-55
 *       if no hit, or not (h.t < max_t_i): stop                                         shading.hpp:33
 *       slot j = h
 *       m = (float)((double)h.t + step)                                                 shading.hpp:32
 *
 * With min_t = (float)(0.0 + 1e-3) and step = 1e-3 this is the list of occluders that shadow_intensity(ray, max_t)
 * visits until its sum saturates: the running float sum of 1 - transparency over a list, clamped at 1 where it reaches 1,
 * is ctr_cast_rays' CTR_RAY_SHADOW bit for bit (as long as the list did not fill all K slots first).  Every cast is
 * ctr_cast_rays' nearest-hit cast: every object in scene order, ties on t to the lower object index (inside a mesh to the
 * lower file index), the mesh's AABB test first, the same hit record (point, normal, texture coordinates: the sphere's
 * within 1e-4 of the host's atan2f / asinf, everything else bit-identical to the reference compiled for the host).
 *
 * What the reference's rules mean for a list (they are kept, not worked around):
 *   - a second surface less than `step` behind a listed hit, measured along the ray in the units of t, is skipped: a plane
 *     coincident with a listed one is never listed, and of two objects at the same t the one ray_cast prefers is;
 *   - t is in the reference's mixed units: a sphere measures along dir / |dir|, every other object along dir
 *     (default_schema.hpp:226-251), so `step` and max_t are in those units too, and a list is ordered by t, not by
 *     distance, where dir is not of unit length and spheres are mixed with other objects;
 *   - with step = 0 progress still holds, because ray_cast accepts only dist > min_dist (ray_cast.hpp:43).  But ray_cast
 *     counts a mesh only with its NEAREST valid t (default_schema.hpp:127-143, valid: min_dist <= t), and that strict >
 *     then rejects the mesh whole when this t equals min_dist: after a mesh hit at t the next cast, from min_dist = t,
 *     does not see the mesh at all, and its farther layers vanish from the list;
 *   - t strictly increases along a list;
 *   - exactness of the default walk and of CTR_HITS_LINEAR is ctr_cast_rays', cast by cast: the BVH's culling is exact
 *     except for a ray that lies in a triangle's plane to within rounding; CTR_HITS_LINEAR is exact for every ray.
 * Rays with NaN, infinite or all-zero components get the reference's answer cast by cast (as a rule an empty list) and do
 * not disturb the other rays of their batch.
 *
 * One lane walks one ray's whole chain: a wave runs as long as its longest chain while the lanes that have finished idle.
 *
 * The contract is ctr_cast_rays': asynchronous on `hip_stream`, no allocation, no synchronisation (capturable into a
 * graph), no per-handle scratch (later renders and their counters are undisturbed); calls on one handle are ordered by
 * the caller against the calls that rewrite device arrays.
 */
#ifndef CUTRACE_HITS_H
#define CUTRACE_HITS_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_HITS_IGNORE_TRANSPARENT 1u /* every cast with ignore_transparent = true, as CTR_RAY_IGNORE_TRANSPARENT */
#define CTR_HITS_LINEAR 2u             /* walk meshes linearly, as CTR_RAY_LINEAR                                   */
#define CTR_HITS_MAX 65535u            /* the largest max_hits                                                      */

typedef struct ctr_hit_query {
  uint64_t n_rays;        /* < 2^31; 0: nothing is launched                                                         */
  uint32_t flags;         /* CTR_HITS_*                                                                             */
  uint32_t max_hits;      /* K: 1 .. CTR_HITS_MAX                                                                   */
  float min_t;            /* every ray's first min_dist when d_min_t is NULL                                        */
  float max_t;            /* every ray's max_dist when d_max_t is NULL; may be +inf                                 */
  double step;            /* the reference's 1e-3 (shading.hpp:32); finite, >= 0                                    */
  const float *d_origin;  /* n x 3, device memory of the scene's device (as every pointer below)                   */
  const float *d_dir;     /* n x 3, need not be normalised                                                          */
  const float *d_min_t;   /* optional: n per-ray first min_dist values                                              */
  const float *d_max_t;   /* optional: n per-ray max_dist values                                                    */
  /* outputs, each optional (NULL = not written), at least one required:                                            */
  int32_t *d_count;       /* n: slots filled for the ray, 0 .. K                                                    */
  /* per-slot outputs, SLOT-MAJOR: slot j of ray i at element j * n + i, so that slot j of all rays is one contiguous
   * batch of n.  Slots count .. K-1 of a ray hold what ctr_cast_rays writes on a miss.                             */
  float *d_t;             /* K x n: distance, +inf in an unfilled slot                                              */
  int32_t *d_object;      /* K x n: index into ctr_scene_desc.objects, -1 in an unfilled slot                       */
  int32_t *d_prim;        /* K x n: a mesh hit's triangle, file order within the mesh; -1 otherwise                 */
  float *d_point;         /* K x n x 3: hit point (0, 0, 0 in an unfilled slot)                                     */
  float *d_normal;        /* K x n x 3: the reference's normal (0, 0, 0 in an unfilled slot)                        */
  float *d_uv;            /* K x n x 2: texture coordinates as ctr_render_uv gives them (0, 0 in an unfilled slot)  */
} ctr_hit_query;

/* Lists the hits of q->n_rays rays on `hip_stream` (NULL: the null stream of the scene's device).  d_count alone is a
 * valid query: counting needs no slot memory.  CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched,
 * for: a NULL scene or query; NULL rays when n_rays > 0; unknown flag bits; max_hits 0 or above CTR_HITS_MAX; a step that
 * is negative, NaN or infinite; no output at all; n_rays >= 2^31; with any per-slot output, n_rays * max_hits >= 2^31; a
 * pointer that is not device memory of the scene's device. */
int ctr_list_hits(ctr_scene *scene, const ctr_hit_query *q, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
