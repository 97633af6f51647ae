/*
 * cutrace_nearest.h — nearest-point queries: the closest surface point to each caller-supplied point, against a scene
 * uploaded with ctr_scene_create.
 *
 * The ray queries (cutrace_rays.h, cutrace_hits.h) answer what lies along a ray; this one answers how far a point is from
 * the scene and where the scene is nearest (Embree's rtcPointQuery, Open3D's compute_closest_points): distance fields,
 * snapping, contacts — and, with ctr_inside_points (cutrace_inside.h), a sign for the distance.  For point i:
 *
 *   every admitted object yields a candidate (d2, q): the squared distance and the closest point on the object
 *       triangle (stand-alone or of a mesh): the closest point of the triangle, Ericson's region test
 *       sphere: on the surface, |(|p - c|) - |R||          plane: the foot of the perpendicular
 *   the answer is the minimum of (d2, object index) — inside a mesh of (d2, file index): ctr_cast_rays' tie rules —
 *   over the candidates with d2 <= max_dist_i^2 and d2 finite
 *
 * cutrace_amd/csrc/nearest_point.h is the definition, operation by operation in float; the answer is THAT arithmetic's, bit for
 * bit, whichever way the meshes are walked.  A mesh is walked through its four-wide BVH with a distance bound per box that is
 * conservative in float, so the default walk and CTR_NEAREST_LINEAR give the same bits.  The distance is
 * within 8 * 2^-24 * (distance + the triangle's largest edge + |p - A|) of the exact one (A: a corner of the triangle; four times
 * the worst case a search found).
 *
 * A point with a NaN or an infinity in it, a per-point max_dist that is NaN or negative, and a point farther than max_dist from
 * everything admitted get the miss values of ctr_cast_rays and do not disturb the other points of their batch.  The surface is
 * the scene's as it is now: every edit of the handle (cutrace_update.h, cutrace_rebuild.h, cutrace_replace.h, cutrace_topology.h,
 * cutrace_objects.h) is seen by the next query.
 *
 * The contract is ctr_cast_rays': asynchronous on `hip_stream`, no allocation, no synchronisation (capturable into a
 * graph), no per-handle scratch; calls on one handle are ordered by the caller against the calls that rewrite device arrays.
 */
#ifndef CUTRACE_NEAREST_H
#define CUTRACE_NEAREST_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_NEAREST_LINEAR 1u      /* every triangle of every admitted mesh, no tree: the cross-check of the default walk  */
#define CTR_NEAREST_SKIP_PLANES 2u /* planes are no candidates (a room's walls otherwise win almost everywhere)            */

typedef struct ctr_nearest_query {
  uint64_t n_points;        /* < 2^31; 0: nothing is launched                                                        */
  uint32_t flags;           /* CTR_NEAREST_*                                                                         */
  int32_t object;           /* -1: every object; otherwise only this index into ctr_scene_desc.objects               */
  float max_dist;           /* every point's limit when d_max_dist is NULL; >= 0, may be +inf                        */
  uint32_t reserved;        /* 0                                                                                     */
  const float *d_point;     /* n x 3, device memory of the scene's device (as every pointer below)                   */
  const float *d_max_dist;  /* optional: n per-point limits (a NaN or a negative one: that point misses)             */
  /* outputs, each optional (NULL = not written), at least one required:                                             */
  float *d_distance;        /* n: sqrtf(d2), +inf on a miss                                                          */
  int32_t *d_object;        /* n: index into ctr_scene_desc.objects, -1 on a miss                                    */
  int32_t *d_prim;          /* n: a mesh's triangle, file order within the mesh; -1 otherwise                        */
  float *d_nearest;         /* n x 3: the closest point q (0, 0, 0 on a miss)                                        */
  float *d_normal;          /* n x 3: what ctr_cast_rays reports for a hit there: the triangle's geometric normal, the
                               plane's stored normal, normalize(q - c) for a sphere (0, 0, 0 on a miss)              */
} ctr_nearest_query;

/* Answers q->n_points points on `hip_stream` (NULL: the null stream of the scene's device).  CTR_E_INVALID, with a
 * ctr_last_error message, before the GPU is touched, for: a NULL query; unknown flag bits; no output at all; a max_dist that
 * is negative or NaN; a NULL scene; n_points >= 2^31; NULL points when n_points > 0; an object outside [-1, object count); a
 * pointer that is not device memory of the scene's device. */
int ctr_nearest_points(ctr_scene *scene, const ctr_nearest_query *q, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
