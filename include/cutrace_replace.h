/*
 * cutrace_replace.h — mesh replaces: another triangle COUNT for a mesh of a live scene handle.
 *
 * ctr_scene_update_mesh (cutrace_update.h) and ctr_scene_rebuild_mesh (cutrace_rebuild.h) keep a mesh's topology: the count
 * and the file order of its triangles.  An isosurface extracted anew every step, a level-of-detail switch, a fractured or
 * remeshed body, a cloth that tears have another count each time, and without this call they pay for ctr_scene_destroy +
 * ctr_scene_create: the host's SAH build of every mesh, new page-locked buffers, a tile history that starts over.
 *
 * A replace is a rebuild at a new size.  The mesh's range of the triangle array stays where it is while the new count fits
 * it and moves to the end of the array, with room to grow into, when it does not; the node range follows the same rule.
 * The ranges left behind are dead: nothing names them, and they are released with the handle.  Everything else of the
 * handle stays: its buffers, its tile history, the other meshes and their guard state.
 *
 * Not for ctr_multi groups, and not for empty meshes in either direction: a mesh of no triangles has no place in the
 * top-level tree, and giving it one changes that tree's shape.  CTR_ABI_VERSION is unchanged: the call is an addition.
 */
#ifndef CUTRACE_REPLACE_H
#define CUTRACE_REPLACE_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_REPLACE_HOST 1u   /* the host's binned-SAH builder instead of the device's linear BVH */

typedef struct ctr_replace_info {
  uint32_t builder, fell_back, node_count, levels;   /* as ctr_rebuild_info */
  uint32_t nodes_moved, tris_moved;                  /* 1: that range lives at the end of its array now */
  uint32_t tri_cap;                                  /* triangle records the mesh's range has room for now */
  uint32_t reserved;
} ctr_replace_info;                                  /* 32 bytes */

/* Replace the triangles of mesh `object` by the `n_tris` triangles at `tris`, in host memory or in memory of the scene's
 * device (read in place, after whatever `hip_stream` holds), and give the mesh a tree over them.  n_tris is 1 .. 0xFFFFFF,
 * the limit of a mesh at ctr_scene_create, and may equal the mesh's current count: the call then is ctr_scene_rebuild_mesh
 * in effect.  `flags` is 0 or CTR_REPLACE_HOST, any other bit is rejected; `info`, when not NULL, says what was built and
 * what moved.  The call returns when the handle is consistent again.  Afterwards every render and every query on the handle
 * gives, bit for bit, what a handle created from the same description with this mesh's triangles replaced, and its box set
 * to ctr_mesh_bounds of them, would give; ctr_scene_get_object reports the new count, and ctr_scene_update_mesh and
 * ctr_scene_rebuild_mesh take the new count and refuse the old.  Graphs captured before the call must be captured again.  As
 * after an update, the handle no longer walks the merged tree.
 * Rejected: n_tris == 0, an object that is not a mesh or is an empty mesh now, a vertex that is not finite, memory that is
 * neither the host's nor the scene's device's, a count the record array cannot address.  Every check and every allocation
 * comes before the first write: a rejected or failed call leaves the scene answering as it did. */
int ctr_scene_replace_mesh(ctr_scene *scene, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags,
                           ctr_replace_info *info, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
