/*
 * cutrace_rays.h — cast and shade caller-supplied rays, and shade caller-supplied surface points (ctr_shade_points, below),
 * against a scene uploaded with ctr_scene_create.
 *
 * ctr_cast_rays answers per ray what the reference answers for its own rays:
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
 * Directions of any length: the BVH's box test runs on the direction scaled by a power of two to unit size (and min_t
 * and the distance limit with it), so the default walk decides for dir * 2^j what it decides for dir.  Checked bit for
 * bit from 2^-104 to 2^100 and for scenes scaled by 2^-20 to 2^24 (tests/test_gpu_query_ranges.py).  What remains is
 * the reference's own float range: where its products overflow or go denormal (a direction with components below
 * about 2^-110 against triangles a hundredth of a unit across, say) both walks still restate its arithmetic operation
 * for operation, but no test pins them there.  The same holds where min_t * 2^e, e the exponent of the direction's
 * largest component, leaves the float range (a direction of length 2^100 with min_t 2^30, say): the default walk keeps
 * its scaled min_t finite and conservative there, untested.  Rays with NaN, infinite or all-zero components get the reference's
 * answer (as a rule a miss) and do not disturb the other rays of their batch.
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

/*
 * Radiance queries: ctr_shade_rays answers per ray the reference's third per-ray function,
 *
 *   ray_color<S, bounces>(scene, ray, min_t, ambient)                                   inc/shading.hpp:116-154
 *
 * Phong shading over every light (phong, shading.hpp:64-99, with shadow_intensity per light), reflection and
 * transparency recursed to `bounces`, with the render kernel's numerics: for a camera's rays the colours are the
 * render's.  By default the specular term is the render's fast one (within 1e-4 of the reference);
 * CTR_SHADE_EXACT_POW is the render's CTR_VAR_EXACT_POW (IEEE half vector, f64 pow rounded once).  The reference's
 * unit mix is kept: a sphere's distance is measured along dir / |dir| while the child rays of a hit start at
 * start + distance * dir.
 *
 * Exactness is that of ctr_cast_rays, for every cast of the activation tree: the default walk culls each mesh with its
 * BVH, exact except for rays lying in a triangle's plane; eyes, lights and mirror images of the scene's uploaded
 * cameras are guarded, arbitrary origins are not.  CTR_SHADE_LINEAR walks meshes linearly and is
 * exact for every ray, secondary rays included.
 *
 * The contract is ctr_cast_rays': asynchronous on `hip_stream`, no allocation, no synchronisation (capturable into a
 * graph), no per-handle scratch (later renders, their counters and the tile scheduler are undisturbed).
 */
#define CTR_SHADE_LINEAR 1u    /* walk meshes linearly (exact for every ray), as CTR_RAY_LINEAR                   */
#define CTR_SHADE_EXACT_POW 2u /* the specular term and half vector as under CTR_VAR_EXACT_POW                    */

typedef struct ctr_shade_query {
  uint64_t n_rays;        /* < 2^31; 0: nothing is launched                                                       */
  uint32_t flags;         /* CTR_SHADE_*                                                                          */
  int32_t bounces;        /* 0 .. 15 (CTR_MAX_BOUNCES), ray_color's template argument                             */
  float min_t;            /* ray_color's min_t: what the render passes as fudge                                   */
  float ambient;          /* phong's ambient factor (the render passes the camera's)                              */
  const float *d_origin;  /* n x 3, device memory of the scene's device (as every pointer below)                 */
  const float *d_dir;     /* n x 3, need not be normalised                                                        */
  float *d_color;         /* n x 3, required; (0, 0, 0) on a miss (shading.hpp:119)                               */
  /* optional (NULL = not written), the hit of ray_color's FIRST cast (shading.hpp:123):                          */
  float *d_t;             /* n: distance, +inf on a miss                                                          */
  int32_t *d_object;      /* n: index into ctr_scene_desc.objects, -1 on a miss                                   */
  float *d_normal;        /* n x 3: the reference's normal (0, 0, 0 on a miss)                                    */
} ctr_shade_query;

/* Shades q->n_rays rays on `hip_stream` (NULL: the null stream of the scene's device).  CTR_E_INVALID, with a
 * ctr_last_error message, before the GPU is touched, for: a NULL scene or query; NULL rays when n_rays > 0; unknown
 * flag bits; bounces outside [0, 15]; a missing d_color; a pointer that is not device memory of the scene's device;
 * n_rays >= 2^31; a scene whose mesh trees are so deep that the walk's stack and `bounces` frames do not fit one
 * workgroup's 64 KiB of LDS (CTR_SHADE_LINEAR needs no walk stack). */
int ctr_shade_rays(ctr_scene *scene, const ctr_shade_query *q, void *hip_stream);

/*
 * Surface shading queries: ctr_shade_points answers per caller-supplied surface point the reference's fourth per-ray
 * function, the one the three calls above only reach behind a cast,
 *
 *   phong(scene, incoming, hit, hit_id, normal, ambient)                                inc/shading.hpp:64-99
 *
 * the direct lighting of one point over every light, each light with its own shadow loop through the scene
 * (shadow_intensity, shading.hpp:22-45).  Point, normal, view direction (incoming->dir) and material are the caller's:
 * a rasteriser's G-buffer, the vertices or texel centres of a mesh to be baked, probe points in free space, or the
 * output of ctr_cast_rays after the caller changed normals or swapped materials.  Restated operation for operation:
 * final = ambient * diffuse; per light, direction and distance as `sun` and `point_light` give them, the shadow ray
 * {point, direction.normalized()} with max_dist = distance * |direction|, the shadow loop from (float)(0.0 + 1e-3) in
 * steps of a double add, stopping at the first occluder only when every material of the scene is opaque; the lit term
 * is added when shadow < 1.  Numerics are ctr_shade_rays': the render's fast specular term by default,
 * CTR_POINTS_EXACT_POW for the IEEE half vector and the f64 pow rounded once (chosen by itself for a scene outside the
 * fast term's domain).  With d_object, the material is that object's and -1 ("a miss", what ctr_cast_rays writes)
 * gives (0, 0, 0), ray_color's answer: ctr_shade_points on the output of ctr_cast_rays is ctr_shade_rays with
 * bounces = 0, bit for bit.  A material or object index outside its range reads nothing and gives a quiet NaN in all
 * three colour channels (it cannot be checked on the host without a synchronisation).  A zero normal, a zero view
 * direction, a NaN or infinite point and a point exactly at a light get what the reference's arithmetic gives (NaNs
 * where it gives NaNs) and do not disturb the other points of their batch.
 *
 * d_light_shadow receives shadow_intensity towards every light, in light order, a row of n_lights per point — also
 * for the lights whose term is skipped, for a "miss" and for a bad index.
 *
 * Exactness: every ray this call casts ends at a light.  The guard of the BVH culling (guard.h)
 * covers every triangle whose plane holds a point light or is parallel to a sun WHATEVER the ray's origin — a ray
 * towards a light can lie in a triangle's plane only if the light does — so the default walk is exact for every
 * point, not only for guarded origins.  CTR_POINTS_LINEAR is the cross-check (and what a mesh that went linear walks
 * anyway); the tests compare the two bit for bit.
 *
 * The contract is ctr_cast_rays': asynchronous on `hip_stream`, no allocation, no synchronisation (capturable into a
 * graph), no per-handle scratch (later renders, their counters and the tile scheduler are undisturbed).
 */
#define CTR_POINTS_LINEAR 1u    /* walk meshes linearly, as CTR_SHADE_LINEAR                                       */
#define CTR_POINTS_EXACT_POW 2u /* half vector and specular term as under CTR_VAR_EXACT_POW                        */

typedef struct ctr_point_query {
  uint64_t n_points;         /* < 2^31; 0: nothing is launched                                                     */
  uint32_t flags;            /* CTR_POINTS_*                                                                       */
  int32_t material;          /* every point's material when d_material and d_object are both NULL                 */
  float ambient;             /* phong's ambient factor                                                             */
  uint32_t reserved;         /* 0                                                                                  */
  const float *d_point;      /* n x 3: phong's *hit; required when n_points > 0                                    */
  const float *d_normal;     /* n x 3: phong's *normal, need not be unit; required with d_color                    */
  const float *d_view;       /* n x 3: incoming->dir, need not be unit; required with d_color                      */
  const int32_t *d_material; /* optional: n indices into ctr_scene_desc.materials                                  */
  const int32_t *d_object;   /* optional: n indices into ctr_scene_desc.objects, -1 = a miss; excludes d_material  */
  float *d_color;            /* n x 3                                                                              */
  float *d_light_shadow;     /* n x n_lights, row per point: shadow_intensity towards each light, in light order   */
} ctr_point_query;

/* Shades q->n_points points on `hip_stream` (NULL: the null stream of the scene's device).  d_color and d_light_shadow
 * are each optional, one of them is required; when only d_light_shadow is asked for, d_normal, d_view and the material
 * inputs may be NULL and are not read.  CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for: a
 * NULL scene or query; a NULL d_point when n_points > 0; unknown flag bits; no output at all; d_color without d_normal
 * or d_view; both d_material and d_object; a scalar `material` outside [0, n_materials) when it is the one in use;
 * n_points >= 2^31; a pointer that is not device memory of the scene's device; a scene whose mesh trees are so deep
 * that the walk's stack does not fit one workgroup's 64 KiB of LDS (CTR_POINTS_LINEAR needs none). */
int ctr_shade_points(ctr_scene *scene, const ctr_point_query *q, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
