// mesh_refit.h — the refit of one mesh's four-wide tree (bvh.h DNode4) after its vertices moved: the tree's shape and the
// triangles' leaf order stay, every used slot's box is recomputed bottom-up (include/cutrace_update.h).
//
// Two halves.  The per-slot arithmetic is __host__ __device__: mesh_update.hip runs it one lane per (node, slot), and
// scripts/mesh_update_check.cpp runs the same text on the host against a brute-force min / max.  The LEVEL SCHEDULE is host
// only: the nodes grouped by height, so that one launch per level finds every inner child's boxes already written by an
// earlier launch — no lane ever waits for another.
//
// A box is a min / max of vertex coordinates, so it is exact whatever the order of the operations; only the SIGN of a zero
// can depend on it (fminf(-0, +0) may give either).  A box that differs by the sign of a zero bounds the same points.
#ifndef CUTRACE_AMD_MESH_REFIT_H
#define CUTRACE_AMD_MESH_REFIT_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bvh.h"
#include "scene_device.h"
#include "tri_record.h"

// Slot `c` of node `node` of a mesh gets its box.  nodes: the mesh's first node; recs: its first DTri record (leaf order; only
// `orig` is read); verts: the new vertices, nine floats per triangle in FILE order.  A leaf slot: min / max over the vertices
// of its triangles.  An inner slot: the union of the used slots of that child node, which an EARLIER level has written.  An
// empty slot (BVH_LEAF_FLAG) is left as it is.
CTR_HD inline void refit_slot(DNode4 *nodes, uint32_t node, int c, const DTri *recs, const float *verts) {
  DNode4 &N = nodes[node];
  const uint32_t d = N.child[c];
  if (d == BVH_LEAF_FLAG) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (d & BVH_LEAF_FLAG) {
    const uint32_t first = d & 0xFFFFFFu, count = (d >> 24) & 0x7Fu;
    for (uint32_t k = 0; k < count; k++) {
      const float *v = verts + 9u * (size_t)recs[first + k].orig;
      for (int p = 0; p < 3; p++)
        for (int a = 0; a < 3; a++) {
          lo[a] = fminf(lo[a], v[3 * p + a]);
          hi[a] = fmaxf(hi[a], v[3 * p + a]);
        }
    }
  } else {
    const DNode4 &K = nodes[d];
    for (int s = 0; s < 4; s++) {
      if (K.child[s] == BVH_LEAF_FLAG) continue;
      for (int a = 0; a < 3; a++) {
        lo[a] = fminf(lo[a], K.lo[a][s]);
        hi[a] = fmaxf(hi[a], K.hi[a][s]);
      }
    }
  }
  for (int a = 0; a < 3; a++) { N.lo[a][c] = lo[a]; N.hi[a][c] = hi[a]; }
}

// The mesh's box: the union of the root's used slots — the min / max of all vertices (the reference's per-mesh AABB,
// ctr_mesh_bounds).  box: min (3), max (3).
CTR_HD inline void refit_mesh_box(const DNode4 &root, float *box) {
  for (int a = 0; a < 3; a++) { box[a] = INFINITY; box[3 + a] = -INFINITY; }
  for (int s = 0; s < 4; s++) {
    if (root.child[s] == BVH_LEAF_FLAG) continue;
    for (int a = 0; a < 3; a++) {
      box[a] = fminf(box[a], root.lo[a][s]);
      box[3 + a] = fmaxf(box[3 + a], root.hi[a][s]);
    }
  }
}


// The nodes of one mesh grouped by height: level 0 holds the nodes whose used children are all leaves, level h the nodes
// whose highest inner child sits in level h - 1.  nodes[begin[h] .. begin[h + 1]) are the node indices (relative to the
// mesh's first node) of level h.
struct LevelSchedule {
  std::vector<uint32_t> nodes;
  std::vector<uint32_t> begin;  // levels() + 1 entries
  size_t levels() const { return begin.empty() ? 0 : begin.size() - 1; }
};

// The schedule of the tree nodes[0 .. node_count) (node 0 the root) over `tri_count` triangles.  false — and an empty
// schedule — for a tree the refit kernels must not be given: a child index that is not a LATER node (bvh.cpp emits a
// parent before its children, so this also rules out a cycle), a leaf that reaches past the mesh's triangles, or more
// levels than BVH4_MAX_DEPTH + 1.
inline bool level_schedule(const DNode4 *nodes, uint32_t node_count, uint32_t tri_count, LevelSchedule &out) {
  out = LevelSchedule();
  if (!node_count) return false;
  std::vector<uint32_t> height(node_count, 0u);
  uint32_t top = 0;
  for (uint32_t n = node_count; n-- > 0;) {  // children come after their parent: backwards, every child is done first
    uint32_t h = 0;
    for (int c = 0; c < 4; c++) {
      const uint32_t d = nodes[n].child[c];
      if (d & BVH_LEAF_FLAG) {
        if ((d & 0xFFFFFFu) + ((d >> 24) & 0x7Fu) > tri_count) return false;
      } else {
        if (d <= n || d >= node_count) return false;
        h = std::max(h, height[d] + 1u);
      }
    }
    height[n] = h;
    top = std::max(top, h);
  }
  if (top > BVH4_MAX_DEPTH) return false;
  out.begin.assign(top + 2, 0u);
  for (uint32_t n = 0; n < node_count; n++) out.begin[height[n] + 1]++;
  for (size_t h = 1; h < out.begin.size(); h++) out.begin[h] += out.begin[h - 1];
  out.nodes.resize(node_count);
  std::vector<uint32_t> at(out.begin.begin(), out.begin.end() - 1);
  for (uint32_t n = 0; n < node_count; n++) out.nodes[at[height[n]]++] = n;
  return true;
}

#endif
