/*
 * cutrace_edit.h — live lights and materials: a scene handle's lights or materials replaced without rebuilding it.
 *
 * A moving lamp, a day cycle, a look-dev session turning `reflexivity` or `transparency` up and down do not have to destroy
 * and create the handle: the geometry, its trees, the handle's page-locked buffers, its per-tile cost history and its refit
 * schedules stay.  What an edit re-derives is the records themselves, the flags the choice of kernel build reads (is every
 * material opaque, does any reflect or transmit, is the fast specular path inside the colour tolerance), the "material is
 * transparent" bit of the objects, and the guard of the BVH culling: a point light or a sun is one of its probes, and a flat
 * object whose material reflects is a mirror that adds images of the eyes.  The guard's scan of the triangle planes runs on
 * the GPU when it is large enough to pay for a launch (CUTRACE_GUARD_SCAN=host|device in the environment overrides the
 * choice, per call); either side gives the same guard.
 *
 * Afterwards every render (plain, supersampled, uv, lens, images, batch) and every query (ctr_cast_rays, ctr_shade_rays,
 * ctr_shade_points) on the handle gives, bit for bit, what a handle created from the same description with these lights or
 * materials gives, with the same kernel build (ctr_debug_last_kernel) and the same work counters under CTR_VAR_STATS.
 *
 * The calls are synchronous, like ctr_scene_set_cameras: they wait for the device (hipDeviceSynchronize) before any device
 * array is touched and return when the handle is consistent again.  The device arrays are reused while the new count fits
 * them.  A HIP graph captured on the handle BEFORE an edit must be captured again: kernel arguments carry the counts and the
 * flags by value, and an edit may have moved an array.
 * Not for ctr_multi groups.  CTR_ABI_VERSION is unchanged: the calls are additions.
 *
 * Live objects — a sphere, a plane or a stand-alone triangle moved, any object given another material — are the third edit
 * of this header: cutrace_objects.h, included below, declares them under the same contract.
 */
#ifndef CUTRACE_EDIT_H
#define CUTRACE_EDIT_H

#include <stdint.h>

#include "cutrace_amd.h"
#include "cutrace_objects.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replace the scene's lights.  n_lights may be 0 (lights may then be NULL) and may differ from before.
 * CTR_E_INVALID, with a ctr_last_error message and the handle untouched, for: a NULL scene; NULL lights with n_lights > 0; a
 * light whose type is above CTR_LIGHT_POINT. */
int ctr_scene_set_lights(ctr_scene *scene, const ctr_light *lights, uint64_t n_lights);

/* Replace the scene's materials.  n_materials may differ from before as long as every object's material index stays below it.
 * CTR_E_INVALID, with a ctr_last_error message and the handle untouched, for: a NULL scene; NULL materials with
 * n_materials > 0; a material whose type is not CTR_MAT_PHONG; an object whose material index is not below n_materials. */
int ctr_scene_set_materials(ctr_scene *scene, const ctr_material *materials, uint64_t n_materials);

/* How many lights / materials the handle currently has. */
int ctr_scene_light_count(const ctr_scene *scene, uint64_t *n);
int ctr_scene_material_count(const ctr_scene *scene, uint64_t *n);

/* Test hook: the guard state of mesh `object` (index into the scene's objects).  *n_guarded: how many of its triangles are in
 * its guard records; guarded[0 .. min(capacity, *n_guarded)): their indices in the file, ascending (guarded may be NULL when
 * capacity is 0); *linear: 1 when the mesh is walked linearly (then none is guarded).  CTR_E_INVALID for a NULL scene,
 * n_guarded or linear, or an object that is not a mesh. */
int ctr_debug_guard_state(ctr_scene *scene, uint32_t object, uint32_t *guarded, uint64_t capacity, uint64_t *n_guarded, int *linear);

#ifdef __cplusplus
}
#endif

#endif
