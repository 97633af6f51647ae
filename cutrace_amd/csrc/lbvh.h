// lbvh.h — the SHAPE of a four-wide tree over one mesh's triangles, made quickly: a linear BVH (Morton keys, Karras' binary
// radix tree, a collapse to bvh.h DNode4 descriptors).  include/cutrace_rebuild.h, DESIGN.md §21.
//
// Descriptors only.  A walk's result is the smallest (t, file index) whatever the tree looks like (bvh.h), so the shape is
// free; the boxes are refit_slot's business (mesh_refit.h), level by level, as after any update.
//
// Two halves, as in mesh_refit.h.  The per-lane text is __host__ __device__: mesh_build.hip runs it one lane per triangle
// or per binary node, and scripts/mesh_rebuild_check.cpp runs the same text on the host with std::stable_sort for the sort.
// Every lane reads only the call's input and what an EARLIER launch wrote, and writes only its own element.  The ACCEPTANCE
// is host only: what the device hands back is numbered, compacted and checked before any kernel may walk it.
#ifndef CUTRACE_AMD_LBVH_H
#define CUTRACE_AMD_LBVH_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bvh.h"
#include "mesh_refit.h"
#include "tri_record.h"

#define LBVH_AXIS_BITS 21  // per axis: a 63-bit key

// one node of the binary radix tree over the sorted keys: the positions [first, last] it covers; its left child covers
// [first, split] and is binary node `split` (a single position: that triangle), its right child [split + 1, last], node split + 1
struct LbvhNode { uint32_t first, last, split; };

// the centre of triangle `t`'s box (what bvh.cpp's builders call its centroid), nine floats per triangle at `verts`
CTR_HD inline void lbvh_centroid(const float *verts, uint32_t t, float *c) {
  const float *v = verts + 9u * (size_t)t;
  for (int a = 0; a < 3; a++) {
    const float lo = fminf(v[a], fminf(v[3 + a], v[6 + a])), hi = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
    c[a] = 0.5f * lo + 0.5f * hi;  // (each half first: the sum of two finite floats of one mesh may overflow, the halves' cannot)
  }
}

// bit i of `q` (21 bits) to bit 3 * i
CTR_HD inline uint64_t lbvh_spread(uint64_t q) {
  q &= 0x1FFFFFull;
  q = (q | q << 32) & 0x1F00000000FFFFull;
  q = (q | q << 16) & 0x1F0000FF0000FFull;
  q = (q | q << 8) & 0x100F00F00F00F00Full;
  q = (q | q << 4) & 0x10C30C30C30C30C3ull;
  q = (q | q << 2) & 0x1249249249249249ull;
  return q;
}

// The Morton key of centroid `c` within the centroid bounds lo / hi: 21 bits per axis, x the highest of each triple.  In f64:
// hi - lo of two finite floats cannot overflow there, so no quotient is inf / inf.  An axis of zero extent contributes zero
// bits; a flat or single-point mesh gives keys that are simply equal in those bits, never a NaN.
CTR_HD inline uint64_t lbvh_key(const float *c, const float *lo, const float *hi) {
  uint64_t key = 0;
  for (int a = 0; a < 3; a++) {
    const double ext = (double)hi[a] - (double)lo[a];
    uint64_t q = 0;
    if (ext > 0.0) {
      const double x = ((double)c[a] - (double)lo[a]) / ext * 2097152.0;  // 2^21
      q = x >= 2097151.0 ? 2097151ull : (x > 0.0 ? (uint64_t)x : 0ull);
    }
    key |= lbvh_spread(q) << (2 - a);
  }
  return key;
}

CTR_HD inline int lbvh_clz64(uint64_t x) {
  int n = 0;
  if (!x) return 64;
  for (uint64_t bit = 1ull << 63; !(x & bit); bit >>= 1) n++;
  return n;
}

// Karras' delta: the length of the common prefix of the keys at positions i and j, -1 beyond the array.  Equal keys are told
// apart by their positions, so that a run of equal keys — all of them, for a mesh collapsed to a point — splits in halves.
CTR_HD inline int lbvh_delta(const uint64_t *keys, uint32_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= (int64_t)n) return -1;
  const uint64_t x = keys[i] ^ keys[j];
  return x ? lbvh_clz64(x) : 64 + lbvh_clz64((uint64_t)i ^ (uint64_t)j);
}

// Internal node i < n - 1 of the binary radix tree over n >= 2 sorted keys (Karras 2012): reads the keys, returns its own node.
CTR_HD inline LbvhNode lbvh_node(const uint64_t *keys, uint32_t n, uint32_t i) {
  const int64_t I = i;
  const int d = lbvh_delta(keys, n, I, I + 1) > lbvh_delta(keys, n, I, I - 1) ? 1 : -1;
  const int dmin = lbvh_delta(keys, n, I, I - d);
  int64_t lmax = 2;
  while (lbvh_delta(keys, n, I, I + lmax * d) > dmin) lmax *= 2;  // (ends: delta is -1 beyond the array, and dmin >= -1)
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (lbvh_delta(keys, n, I, I + (l + t) * d) > dmin) l += t;
  const int64_t j = I + l * d;
  const int dnode = lbvh_delta(keys, n, I, j);
  int64_t s = 0;
  for (int64_t div = 2, t = (l + 1) / 2;; div *= 2, t = (l + div - 1) / div) {
    if (lbvh_delta(keys, n, I, I + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int64_t split = I + s * d + (d < 0 ? -1 : 0);
  return LbvhNode{(uint32_t)(I < j ? I : j), (uint32_t)(I < j ? j : I), (uint32_t)split};
}

// a node whose four slots are empty: scene_flatten.h empty_node4(), for either side
CTR_HD inline void lbvh_empty_node(DNode4 &N) {
  for (int c = 0; c < 4; c++) {
    for (int a = 0; a < 3; a++) { N.lo[a][c] = 3.4028235e38f; N.hi[a][c] = 3.4028235e38f; }
    N.child[c] = BVH_LEAF_FLAG;
  }
  N.axis = 0;
  N.pad[0] = N.pad[1] = N.pad[2] = 0;
}

// The DNode4 descriptors of binary node i, written to out[i] (so `out` is sparse: a binary node that some collapse swallowed
// is never referenced).  A child whose range holds at most `leaf` positions becomes a leaf slot (first, count) of the sorted
// order; any other child is expanded into ITS two children, each a leaf slot or an inner slot naming the binary node: two to
// four used slots, in key order, the unused ones last and empty.  n <= leaf: node 0 is one leaf of everything.
// bin: the binary tree of an earlier launch (n >= 2), keys: the sorted keys.  Lanes: max(n - 1, 1).
CTR_HD inline void lbvh_collapse(const LbvhNode *bin, const uint64_t *keys, uint32_t n, uint32_t leaf, uint32_t i, DNode4 *out) {
  DNode4 &N = out[i];  // (written in place: a local node indexed by `used` would live in scratch memory on the device)
  lbvh_empty_node(N);
  if (n <= leaf) {
    if (i == 0) N.child[0] = BVH_LEAF_FLAG | (n << 24);
    return;
  }
  const LbvhNode B = bin[i];
  // (what lbvh_node writes always passes the range tests here and below; they keep every index inside the arrays whatever
  //  `bin` holds, and a node cut short by them is one lbvh_accept refuses)
  if (B.first <= B.split && B.split < B.last && B.last < n && B.last - B.first + 1u > leaf) {
    int used = 0;
    auto put = [&](uint32_t first, uint32_t last, uint32_t node, bool expand) {
      const uint32_t count = last - first + 1u;
      if (count <= leaf) N.child[used++] = BVH_LEAF_FLAG | (count << 24) | first;
      else if (!expand) N.child[used++] = node;
      else return false;
      return true;
    };
    const uint32_t kid[2] = {B.split, B.split + 1u}, kf[2] = {B.first, B.split + 1u}, kl[2] = {B.split, B.last};
    for (int c = 0; c < 2; c++) {
      if (put(kf[c], kl[c], kid[c], true)) continue;
      if (kid[c] >= n - 1u) continue;
      const LbvhNode K = bin[kid[c]];  // (more than `leaf` >= 1 positions: an internal node)
      if (!(K.first <= K.split && K.split < K.last && K.last < n)) continue;
      put(K.first, K.split, K.split, false);
      put(K.split + 1u, K.last, K.split + 1u, false);
    }
    const uint64_t x = keys[B.first] ^ keys[B.last];
    N.axis = x ? (uint32_t)(2 - (63 - lbvh_clz64(x)) % 3) : 0u;  // the highest key bit that differs across the range
  }
}

// ---- host only: what the builder handed back becomes a tree the kernels may be given, or is refused ----

// `sparse[0 .. n_sparse)`: DNode4 descriptors indexed by binary node, node 0 the root; `order`: the sorted file indices, one
// per triangle.  The nodes reachable from the root are numbered so that every child comes after its parent, copied to
// `nodes` in that numbering with their child indices rewritten, and checked: `order` is a permutation of 0 .. n - 1; the
// leaves cover every position exactly once, 1 .. leaf triangles each; level_schedule (mesh_refit.h) accepts the tree — child
// after parent, leaves inside the mesh, at most BVH4_MAX_DEPTH + 1 levels.  false: refused (`nodes` is then meaningless); no
// input, however broken, makes this read out of bounds or loop.  *levels: what the tree would need, also when that is too many.
inline bool lbvh_accept(const DNode4 *sparse, uint32_t n_sparse, const uint32_t *order, uint32_t n, uint32_t leaf, std::vector<DNode4> &nodes,
                        uint32_t *levels = nullptr) {
  nodes.clear();
  if (levels) *levels = 0;
  if (!n || !n_sparse) return false;
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t k = 0; k < n; k++) {
    if (order[k] >= n || seen[order[k]]) return false;
    seen[order[k]] = 1;
  }
  // breadth first from the root: a parent is numbered before its children; a node reached twice is no tree
  std::vector<uint32_t> number(n_sparse, 0xFFFFFFFFu), queue(1, 0u), depth(1, 1u);
  number[0] = 0;
  std::vector<uint8_t> covered(n, 0);
  uint64_t covered_total = 0;
  uint32_t deepest = 1;
  for (size_t q = 0; q < queue.size(); q++) {
    const DNode4 &S = sparse[queue[q]];
    deepest = std::max(deepest, depth[q]);
    for (int c = 0; c < 4; c++) {
      const uint32_t d = S.child[c];
      if (d == BVH_LEAF_FLAG) continue;
      if (d & BVH_LEAF_FLAG) {
        const uint32_t first = d & 0xFFFFFFu, count = (d >> 24) & 0x7Fu;
        if (count < 1 || count > leaf || first >= n || count > n - first) return false;
        for (uint32_t k = first; k < first + count; k++) {
          if (covered[k]) return false;
          covered[k] = 1;
        }
        covered_total += count;
      } else {
        if (d >= n_sparse || number[d] != 0xFFFFFFFFu) return false;
        number[d] = (uint32_t)queue.size();
        queue.push_back(d);
        depth.push_back(depth[q] + 1u);
      }
    }
  }
  if (levels) *levels = deepest;
  if (covered_total != n) return false;
  nodes.resize(queue.size());
  for (size_t q = 0; q < queue.size(); q++) {
    nodes[q] = sparse[queue[q]];
    for (int c = 0; c < 4; c++)
      if (!(nodes[q].child[c] & BVH_LEAF_FLAG)) nodes[q].child[c] = number[nodes[q].child[c]];
  }
  LevelSchedule S;
  return level_schedule(nodes.data(), (uint32_t)nodes.size(), n, S);
}

#endif
