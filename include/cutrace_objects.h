/*
 * cutrace_objects.h — live objects: the parameters of a scene handle's objects replaced without rebuilding it.  Part of
 * cutrace_edit.h, which includes this file; the calls are kept in a header of their own so that each header's list of entry
 * points stays what its tests pin it to.
 *
 * A moving sphere, a sliding or tilting mirror plane, a wall of a room opened, a mesh given another of the materials already
 * loaded do not have to destroy and create the handle: the meshes, their trees, the handle's page-locked buffers, its per-tile
 * cost history and its refit schedules stay.  Topology is fixed in THIS call, as it is for a mesh update: the number of objects and
 * the type of each stay what the handle has (cutrace_topology.h adds and removes objects).  What may change:
 *   sphere               v0 (centre), f0 (radius), mat_idx
 *   plane                v0 (point), v1 (normal), mat_idx
 *   stand-alone triangle v0, v1, v2, mat_idx
 *   mesh                 mat_idx only: tri_count must equal the mesh's count; tri_begin, v0 and v1 are ignored, and the mesh's
 *                        triangles, tree and current box stay what they are (after ctr_scene_update_mesh the box is the refitted
 *                        one, not the box of the description)
 * What an edit re-derives is the object records, the loop over spheres and triangles, the packing of the planes (a plane that
 * becomes or stops being axis-aligned changes which plane records exist, their order and their number), the "material is
 * transparent" bit of the objects, and the guard of the BVH culling: a flat object whose material reflects is a mirror, and its
 * images of the eyes are the guard's probes.
 *
 * Afterwards every render (plain, supersampled, uv, lens, images, batch) and every query (ctr_cast_rays, ctr_shade_rays,
 * ctr_shade_points) on the handle gives, bit for bit, what a handle created from the edited description gives, with the same
 * kernel build (ctr_debug_last_kernel) and the same work counters under CTR_VAR_STATS.
 *
 * ctr_scene_set_objects is synchronous, like ctr_scene_set_lights: it waits for the device (hipDeviceSynchronize) before any
 * device array is touched and returns when the handle is consistent again.  A HIP graph captured on the handle BEFORE an edit
 * must be captured again: kernel arguments carry the counts and the first plane records by value, and an edit may have moved
 * the plane array.
 * Not for ctr_multi groups.  CTR_ABI_VERSION is unchanged: the calls are additions.
 */
#ifndef CUTRACE_OBJECTS_H
#define CUTRACE_OBJECTS_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replace the parameters of the scene's objects (see above for what may change per type).
 * CTR_E_INVALID, with a ctr_last_error message and the handle untouched, for: a NULL scene; NULL objects with n_objects > 0;
 * n_objects different from the handle's count; a type above CTR_OBJ_SPHERE or different from the type the object was created
 * with; a mesh whose tri_count differs; a mat_idx not below the handle's current material count.  Every check runs before the
 * first write.  Values are not validated beyond that, as ctr_scene_create does not validate them: a zero normal, a negative
 * radius and coordinates that are not finite go through as they do there. */
int ctr_scene_set_objects(ctr_scene *scene, const ctr_object *objects, uint64_t n_objects);

/* How many objects the handle has. */
int ctr_scene_object_count(const ctr_scene *scene, uint64_t *n);

/* Object `index` as ctr_scene_set_objects would accept it back unchanged: its type, its current mat_idx and its current
 * parameters; for a mesh the current box in v0 / v1 and tri_count, with tri_begin 0.  So that a caller can edit one field of one
 * object without keeping a mirror of the scene.  CTR_E_INVALID for NULL arguments or an index out of range. */
int ctr_scene_get_object(const ctr_scene *scene, uint64_t index, ctr_object *out);

#ifdef __cplusplus
}
#endif

#endif
