/*
 * cutrace_update.h — mesh updates: new vertices into a live scene handle, the mesh's BVH refitted on the GPU.
 *
 * A ctr_scene whose geometry moves — a skinned or simulated mesh, a turntable, one mesh of sixteen — does not have to be
 * destroyed and created again.  The tree over a mesh's triangles keeps its SHAPE and the triangles keep their places in
 * its leaves; the triangle records are rebuilt from the new vertices and the boxes of the tree are recomputed bottom-up, on
 * the device.  The handle keeps its page-locked buffers and its per-tile cost history.
 *
 * A walk's result is the smallest valid t, ties broken by the triangle's index in the file, whatever the tree looks like.
 * So an updated handle gives, bit for bit, what a freshly created one gives; only the time a walk takes depends on how well
 * the old tree still fits the moved triangles.  When it fits badly — a mesh folded through itself, not a rigid motion —
 * ctr_scene_rebuild_mesh (cutrace_rebuild.h) gives the mesh a new tree on the same handle.
 *
 * Topology is fixed by contract: the triangle count and the file order of the triangles do not change.
 * Not for ctr_multi groups.  CTR_ABI_VERSION is unchanged: the calls are additions.
 */
#ifndef CUTRACE_UPDATE_H
#define CUTRACE_UPDATE_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replace the vertices of mesh `object` (index into the scene's objects; must be a CTR_OBJ_MESH with exactly n_tris
 * triangles, file order).  `tris` is host memory or memory of the scene's device.  Work on the device is queued on
 * `hip_stream`, after whatever produced `tris` there.  The call returns when the handle is consistent again.
 * Afterwards every render and every query on the handle gives, bit for bit, what a handle created from the same description
 * with this mesh's triangles replaced, and its box set to ctr_mesh_bounds of them, would give.
 * After the first update the handle no longer walks the merged tree: CTR_VAR_MERGE is accepted and takes the two-level walk.
 * CTR_E_INVALID, with a ctr_last_error message and the handle untouched, for: a NULL scene or tris; an object index out of
 * range or an object that is not a mesh; an empty mesh; another triangle count than the mesh has; a pointer that is neither
 * host memory nor memory of the scene's device; a vertex coordinate that is NaN or infinite. */
int ctr_scene_update_mesh(ctr_scene *scene, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, void *hip_stream);

/* The mesh's current box (the reference's per-mesh AABB), as the kernels use it: of the description at first, the min / max
 * of the vertices after an update.  CTR_E_INVALID for a NULL argument or an object that is not a mesh. */
int ctr_scene_mesh_box(const ctr_scene *scene, uint32_t object, ctr_vec3 *bb_min, ctr_vec3 *bb_max);

#ifdef __cplusplus
}
#endif

#endif
