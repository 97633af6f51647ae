/*
 * cutrace_inside.h — inside queries: how many surfaces a ray crosses, whether a point lies inside a body, and with that a
 * sign for ctr_nearest_points' distance, against a scene uploaded with ctr_scene_create (Open3D's count_intersections,
 * compute_occupancy and compute_signed_distance).
 *
 * THE CROSSING COUNT of ray (o, d) over the OPEN interval (min_t, max_t) is a sum over the selected primitives.  Each term is
 * decided by its primitive alone, so neither the order of the visits nor the tree can change it:
 *
 *   mesh triangle, stand-alone triangle   1 when the reference's triangle::intersect accepts it (beta >= 0, gamma >= 0,
 *                                         beta + gamma <= 1, t0 finite, min_t <= t0: ctr_cast_rays' arithmetic) and
 *                                         min_t < t0 < max_t.  A mesh's box test (bound_intersects) is NOT part of it.
 *   sphere                                1 for each of the reference's two roots that is finite and lies in (min_t, max_t);
 *                                         the roots are measured along d / |d|, as ctr_list_hits' are
 *   plane                                 1 when t0 is finite and lies in (min_t, max_t)
 *
 * THE SIGNED COUNT is the same sum with each term weighted:
 *
 *   triangle   +1 when alpha = det[a b d] < 0, -1 when alpha > 0.  alpha = -|a x b| (n . d) with n the normal ctr_cast_rays
 *              reports: +1 is a ray that LEAVES through a face whose normal points along it
 *   sphere     +1 for the root dec + sqrt (the way out), -1 for dec - sqrt (the way in)
 *   plane      +1 when d . n > 0, -1 otherwise
 *
 * For a closed mesh with outward normals and an origin off the surface the signed count over (0, +inf) is the winding number,
 * and the parity of the count is containment.
 *
 * THE EDGE RULE.  The reference's triangle test is inclusive on its edges, so a ray through an edge or a vertex that two or
 * more triangles share may be counted by every one of them, by one, or by none: a single ctr_count_crossings ray through an edge
 * is NOT a parity oracle.  (A watertight rule needs shared vertices; the triangle records keep each triangle on its own.)
 *
 * A POINT IS INSIDE when more than half of R rays from it, R odd, over (0, +inf), counting the selected meshes and spheres
 * only, report an odd count.  The vote is what ctr_inside_points promises: a ray that grazes an edge is outvoted by the
 * others.  The default R = 3 directions (ctr_inside_default_dirs) are, as the float literals the library holds,
 *
 *     ( 0.3713907f,  0.5570860f,  0.7427814f)
 *     (-0.6396021f,  0.7462025f, -0.1842720f)
 *     ( 0.8017837f, -0.2672612f, -0.5345225f)
 *
 * every component non-zero (no direction is parallel to an axis), no two parallel or opposite.  A point with a NaN or an
 * infinity in it is not inside and gets 0 votes.  A body is what a closed surface bounds: an open mesh, or one that holds
 * every triangle twice, has no inside, and the vote then says whatever the parities say.
 *
 * The contract is ctr_cast_rays': asynchronous on `hip_stream`, no allocation, no synchronisation (capturable into a
 * graph), no per-handle scratch; calls on one handle are ordered by the caller against the calls that rewrite device arrays.
 * Both walks visit a mesh's tree from its root with nothing pruned by distance; the *_LINEAR flags test every triangle of
 * every selected mesh instead and give the same integers.
 */
#ifndef CUTRACE_INSIDE_H
#define CUTRACE_INSIDE_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_CROSS_LINEAR 1u         /* every triangle of every selected mesh, no tree: the cross-check of the default walk */
#define CTR_CROSS_SKIP_PLANES 2u    /* planes are not counted                                                             */
#define CTR_CROSS_SKIP_TRIANGLES 4u /* stand-alone triangles are not counted (a mesh's triangles always are)              */

typedef struct ctr_crossing_query {
  uint64_t n_rays;       /* < 2^31; 0: nothing is launched                                                          */
  uint32_t flags;        /* CTR_CROSS_*                                                                             */
  int32_t object;        /* -1: every object; otherwise only this index into ctr_scene_desc.objects                 */
  float min_t, max_t;    /* every ray's open interval when d_min_t / d_max_t is NULL                                */
  const float *d_origin; /* n x 3, device memory of the scene's device (as every pointer below)                     */
  const float *d_dir;    /* n x 3; need not be normalised                                                           */
  const float *d_min_t;  /* optional: n per-ray lower ends                                                          */
  const float *d_max_t;  /* optional: n per-ray upper ends (a NaN end admits nothing)                               */
  /* outputs, each optional (NULL = not written), at least one required:                                            */
  int32_t *d_count;      /* n: the crossing count                                                                   */
  int32_t *d_signed;     /* n: the signed count                                                                     */
} ctr_crossing_query;

/* Counts the crossings of q->n_rays rays on `hip_stream` (NULL: the null stream of the scene's device).  A ray with a
 * non-finite origin, or a NaN, an infinity or three zeros for a direction, gets 0 / 0 and does not disturb the others.
 * CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for: a NULL query; unknown flag bits; no output at
 * all; a NULL scene; n_rays >= 2^31; NULL rays when n_rays > 0; an object outside [-1, object count); a pointer that is not
 * device memory of the scene's device. */
int ctr_count_crossings(ctr_scene *scene, const ctr_crossing_query *q, void *hip_stream);

#define CTR_INSIDE_LINEAR 1u   /* every triangle of every selected mesh, no tree */
#define CTR_INSIDE_MAX_DIRS 15u

typedef struct ctr_inside_query {
  uint64_t n_points;     /* < 2^31; 0: nothing is launched                                                          */
  uint32_t flags;        /* CTR_INSIDE_*                                                                            */
  int32_t object;        /* -1: every mesh and sphere; otherwise ONE mesh or ONE sphere (a plane or a stand-alone
                            triangle bounds nothing and is refused)                                                 */
  uint32_t n_dirs;       /* R: odd, 1 .. CTR_INSIDE_MAX_DIRS; 0: the default table, R = 3                           */
  uint32_t reserved;     /* 0                                                                                       */
  const float *dirs;     /* HOST memory, n_dirs x 3, read before the call returns (copied into the launch); finite and
                            not all zero each; ignored when n_dirs = 0                                              */
  const float *d_point;  /* n x 3, device memory of the scene's device (as every pointer below)                     */
  /* outputs, each optional (NULL = not written), at least one required:                                            */
  uint8_t *d_inside;     /* n: 1 where more than half of the R rays report an odd count, else 0                     */
  uint8_t *d_votes;      /* n: the number of rays that report an odd count; asking for it casts all R rays of every
                            point (without it a wave stops at the first ray after which all its points are decided) */
  float *d_distance;     /* n, IN and OUT: element i is negated where point i is inside (an infinite or NaN element stays
                            as it is: a point farther than ctr_nearest_points' max_dist has no sign)                */
} ctr_inside_query;

/* Decides q->n_points points on `hip_stream`.  CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for:
 * a NULL query; unknown flag bits; n_dirs even or above CTR_INSIDE_MAX_DIRS; NULL dirs with n_dirs > 0; a direction that is not
 * finite or is all zero; no output at all; a NULL scene; n_points >= 2^31; NULL points when n_points > 0; an object outside
 * [-1, object count) or one that is a plane or a stand-alone triangle; a pointer that is not device memory of the scene's
 * device. */
int ctr_inside_points(ctr_scene *scene, const ctr_inside_query *q, void *hip_stream);

/* The default table: three directions, x y z each. */
void ctr_inside_default_dirs(float out[9]);

#ifdef __cplusplus
}
#endif

#endif
