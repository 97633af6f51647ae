/*
 * cutrace_topology.h — a live object COUNT: objects added to and removed from a scene handle.
 *
 * Lights and materials change count and value (cutrace_edit.h), spheres, planes and stand-alone triangles move
 * (cutrace_objects.h), a mesh takes new vertices, a new tree or a new triangle count (cutrace_update.h, cutrace_rebuild.h,
 * cutrace_replace.h).  These calls change the object list itself: a simulation that spawns or despawns a sphere, a body that
 * fractures into a second mesh, an editor that deletes a wall, a scene that starts with no mesh and gains one — without
 * ctr_scene_destroy + ctr_scene_create, which rebuilds every tree on the host and throws away the handle's page-locked
 * buffers, its tile history and its refit schedules.
 *
 * The contract is the other edits': after any sequence of these calls every render and every query on the handle gives, bit
 * for bit, what a handle created from the edited description gives — the removed objects deleted, the added ones appended
 * in call order — the indices in ctr_cast_rays' `object` output included.  Ties go to the lower object index, so an
 * appended object loses them exactly as the last object of a description does.  The kernel build, the launch shape, the
 * room facts and every mesh's guard state are the fresh handle's too, and so are the work counters when every tree on the
 * handle is the host builder's own.  As after a mesh update the merged tree is retired once the object list has changed:
 * CTR_VAR_MERGE is accepted and takes the two-level walk.
 *
 * Ranges.  A removed mesh leaves its range of the triangle array and its range of the node array behind, a removed
 * stand-alone triangle its one record.  ctr_scene_add_mesh takes, per array, the lowest-addressed range left behind that
 * has enough room — whole: ranges are neither split nor merged — and appends a range of exactly the room needed when none
 * fits; ctr_scene_add_object takes a single record left behind for a triangle.  A steady add / remove of equal things
 * therefore stops growing the arrays after its first round.  ctr_scene_room reports the totals.
 *
 * Every call is synchronous in the sense of ctr_scene_set_objects: it waits for the device before it touches an array and
 * returns when the handle is consistent; a HIP graph captured before the call must be captured again.  Every refusal —
 * CTR_E_INVALID with a ctr_last_error message for a NULL argument, an index out of range, a type above CTR_OBJ_SPHERE, a
 * material index not below the current material count, unknown flag bits, a triangle count of 0 or above the limit, a
 * vertex that is not finite, a pointer that is neither host memory nor memory of the scene's device — and every failed
 * allocation comes before the first write and leaves the scene answering as it did.
 *
 * Not for ctr_multi groups.  CTR_ABI_VERSION is unchanged: the calls are additions.
 */
#ifndef CUTRACE_TOPOLOGY_H
#define CUTRACE_TOPOLOGY_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_ADD_HOST 1u   /* the host's binned-SAH builder instead of the device's linear BVH (as CTR_REPLACE_HOST) */

typedef struct ctr_add_info {
  uint32_t index;                                    /* the new object's index: the object count before the call */
  uint32_t builder, fell_back, node_count, levels;   /* as ctr_replace_info */
  uint32_t tris_reused, nodes_reused;                /* 1: the range is one a removed object left behind */
  uint32_t tri_cap;                                  /* triangle records the mesh's range has room for */
} ctr_add_info;                                      /* 32 bytes */

/* (a struct tag beside a function of the same name, as stat has it: a typedef would collide with the function in C) */
struct ctr_scene_room {
  uint64_t tris_live, tris_total;                    /* triangle records inside a range some object owns; in the array */
  uint64_t nodes4_live, nodes4_total;                /* the same of the per-mesh tree nodes */
};                                                   /* 32 bytes */

/* Append a sphere, a plane or a stand-alone triangle, with the fields ctr_scene_set_objects reads.  Its index is the object
 * count before the call and is stored in *index when `index` is not NULL.  A CTR_OBJ_MESH is refused: ctr_scene_add_mesh. */
int ctr_scene_add_object(ctr_scene *scene, const ctr_object *object, uint64_t *index);

/* Append a mesh of the `n_tris` triangles at `tris` (1 .. 0xFFFFFF), in host memory or in memory of the scene's device (read
 * in place, after whatever `hip_stream` holds), with material `mat_idx`.  `flags` is 0 or CTR_ADD_HOST.  The rest of the
 * contract is ctr_scene_replace_mesh's: the finiteness check, the two builders, the fallback to the host's builder that
 * `fell_back` reports, and the limit on the scene's triangle records.  `info`, when not NULL, says what was built and where. */
int ctr_scene_add_mesh(ctr_scene *scene, uint64_t mat_idx, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags,
                       ctr_add_info *info, void *hip_stream);

/* Remove object `index`, of any type, an empty mesh included.  The objects behind it move down by one index, as in a list. */
int ctr_scene_remove_object(ctr_scene *scene, uint64_t index);

/* How much of the triangle and node arrays is in use: `*_total` the records of the arrays, `*_live` those inside a range
 * some object currently owns — a mesh's capacity and its spare records, a stand-alone triangle's record. */
int ctr_scene_room(const ctr_scene *scene, struct ctr_scene_room *out);

#ifdef __cplusplus
}
#endif

#endif
