/*
 * cutrace_rebuild.h — mesh rebuilds: new vertices into a live scene handle AND a new tree over them, its shape built on the GPU.
 *
 * ctr_scene_update_mesh (cutrace_update.h) keeps the shape of a mesh's tree and refits its boxes.  That is the cheapest call
 * for a rigid or nearly rigid motion, and it decays with every frame of a cloth, a fluid surface or a long twist: the boxes
 * grow around triangles that no longer lie where the tree's shape put them.  A rebuild gives the mesh a tree made for the
 * vertices it has now, on the handle it lives in: page-locked buffers, tile history and device arrays stay.
 *
 * The shape comes from a linear BVH built on the device (Morton keys of the triangles' centroids, a radix sort, Karras'
 * binary radix tree, a collapse to four-wide nodes), or, on request, from the host's binned-SAH builder that
 * ctr_scene_create uses.  Either way the boxes are then made by the refit, and the rest is an update.  A walk's result is
 * the smallest valid t, ties broken by the triangle's index in the file, whatever the tree looks like: a rebuilt handle
 * gives, bit for bit, what a freshly created one gives.  Only the time a walk takes depends on the builder.
 *
 * Topology is fixed by contract: the triangle count and the file order of the triangles do not change.
 * Not for ctr_multi groups.  CTR_ABI_VERSION is unchanged: the call is an addition.
 */
#ifndef CUTRACE_REBUILD_H
#define CUTRACE_REBUILD_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_REBUILD_HOST 1u   /* build with the host's binned-SAH builder instead of on the device */

typedef struct ctr_rebuild_info {
  uint32_t builder;     /* 0: the device built the shape, 1: the host did */
  uint32_t fell_back;   /* 1: the device's tree was refused by the host's checks and the host built instead */
  uint32_t node_count, levels;
  uint32_t moved;       /* 1: the tree did not fit the mesh's node range and lives in a new range */
  uint32_t reserved[3];
} ctr_rebuild_info;

/* Replace the vertices of mesh `object` and give it a new tree.  Arguments, memory kinds, stream and rejections are those of
 * ctr_scene_update_mesh; `flags` is 0 or CTR_REBUILD_HOST, any other bit is rejected; `info`, when not NULL, says what was
 * built.  The call returns when the handle is consistent again.  Afterwards every render and every query on the handle
 * gives, bit for bit, what a handle created from the same description with this mesh's triangles replaced, and its box set
 * to ctr_mesh_bounds of them, would give.  Graphs captured before the call must be captured again.  As after an update, the
 * handle no longer walks the merged tree.
 * A tree the device built is checked on the host before any kernel walks it (every triangle in exactly one leaf, every child
 * after its parent, no more levels than the walk's stack holds); one that is refused — keys that peel off one triangle per
 * level make such a tree — is not an error: the host builder runs instead and info->fell_back says so.
 * Every check and every allocation comes before the first write: a rejected or failed call leaves the handle untouched. */
int ctr_scene_rebuild_mesh(ctr_scene *scene, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags,
                           ctr_rebuild_info *info, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
