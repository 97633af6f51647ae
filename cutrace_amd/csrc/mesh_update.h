// mesh_update.h — the launchers of mesh_update.hip: the device half of ctr_scene_update_mesh (include/cutrace_update.h).
// Each returns a hipError_t as int and queues its work on `stream`; none of them waits.
#ifndef CUTRACE_AMD_MESH_UPDATE_H
#define CUTRACE_AMD_MESH_UPDATE_H

#include <stdint.h>

#include "bvh.h"
#include "scene_device.h"

// *flag (one word, zeroed on the stream first) becomes 1 if any of the `n` floats at `v` is NaN or infinite
int ctr_launch_all_finite(const float *v, uint64_t n, uint32_t *flag, void *stream);

// One lane per leaf-order record k < n of one mesh: from the nine floats of file triangle recs[k].orig at `verts`, the DTri
// record recs[k] (orig kept), the geometric normal gn[4 * orig ..] (FILE order; gn: the mesh's first entry) and the guard's
// seven doubles planes[7 * k ..] — tri_record.h on the device.
int ctr_launch_update_tris(DTri *recs, float *gn, double *planes, const float *verts, uint32_t n, void *stream);

// One lane per (node, slot) of one level of the mesh's schedule (mesh_refit.h): sched[0 .. n_nodes) are the level's node
// indices relative to `nodes`, the mesh's first node.  Launch level after level, lowest first, on ONE stream.
int ctr_launch_refit_level(DNode4 *nodes, const uint32_t *sched, uint32_t n_nodes, const DTri *recs, const float *verts, void *stream);

// box[0..5] = the union of the root's used slots (min, max), after the last level
int ctr_launch_mesh_box(const DNode4 *nodes, float *box, void *stream);

#endif
