// mesh_build.h — the launchers of mesh_build.hip: the device builder of ctr_scene_rebuild_mesh (include/cutrace_rebuild.h), the
// per-lane text of lbvh.h on the device.  Each returns a hipError_t as int and queues its work on `stream`; none of them waits,
// none of them writes anything of the scene: everything goes into scratch buffers of the handle.
#ifndef CUTRACE_AMD_MESH_BUILD_H
#define CUTRACE_AMD_MESH_BUILD_H

#include <stddef.h>
#include <stdint.h>

#include "bvh.h"
#include "lbvh.h"
#include "scene_device.h"

// floats the first launch of the centroid bounds needs at `partials`: six per block
size_t ctr_lbvh_partial_floats(uint32_t n);
// bounds[0..5] = min (3), max (3) of the centroids of the `n` triangles at `verts` (nine floats each, file order): two launches,
// per-block partial min / max, then one block over the partials.  No float atomics.
int ctr_launch_lbvh_bounds(const float *verts, uint32_t n, float *partials, float *bounds, void *stream);
// keys[t] = the 63-bit Morton key of triangle t's centroid within `bounds`, index[t] = t
int ctr_launch_lbvh_keys(const float *verts, uint32_t n, const float *bounds, uint64_t *keys, uint32_t *index, void *stream);
// the bytes of temporary storage the sort of `n` pairs asks for
int ctr_lbvh_sort_temp_bytes(uint32_t n, size_t *bytes);
// (keys_in, index_in) sorted by key into (keys_out, index_out), stable: equal keys keep their file order
int ctr_lbvh_sort(void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *index_in, uint32_t *index_out,
                  uint32_t n, void *stream);
// bin[i], i < n - 1: Karras' binary radix tree over the sorted keys (nothing to do for n < 2)
int ctr_launch_lbvh_tree(const uint64_t *keys, uint32_t n, LbvhNode *bin, void *stream);
// out[i], i < max(n - 1, 1): the DNode4 descriptors of binary node i (lbvh.h lbvh_collapse), leaves of at most `leaf` triangles
int ctr_launch_lbvh_collapse(const LbvhNode *bin, const uint64_t *keys, uint32_t n, uint32_t leaf, DNode4 *out, void *stream);
// recs[k].orig = order[k], k < n: the records take a new leaf order (everything else of them is update_tris' to write)
int ctr_launch_set_orig(DTri *recs, const uint32_t *order, uint32_t n, void *stream);

#endif
