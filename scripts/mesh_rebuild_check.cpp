// mesh_rebuild_check.cpp — the host-checkable half of ctr_scene_rebuild_mesh (include/cutrace_rebuild.h) without a device; meant to
// run under ASan/UBSan as well.  tests/test_mesh_rebuild_cpu.py builds and runs it and reads the lines it prints.
//
//   lbvh       the builder's text (cutrace_amd/csrc/lbvh.h) on the host, std::stable_sort for the sort, over random and degenerate
//              triangle sets: lbvh_accept takes the tree; every triangle in exactly one leaf of 1 .. BVH_LEAF; every child after
//              its parent; level_schedule accepts it; after refit_slot every box is the min / max of what lies below it
//   staircase  63 triangles whose keys peel off one per split: more levels than the walk's stack holds, and lbvh_accept says no
//   broken     descriptors that are no tree (a cycle, a shared child, an uncovered triangle, a leaf past the mesh, an index past
//              the array, an order that is no permutation) are refused without a read out of bounds
//   install    mesh_rebuilt (scene_flatten.cpp) with the update's steps behind it, against flatten_scene of the same triangles:
//              bvh4_build's own tree in place, byte for byte; a tree of more nodes moved to a new range, the other mesh
//              untouched; the LBVH text's tree with the guard's FILE indices and ray_slots; the in-plane cases of
//              mesh_update_check.cpp through rebuilds
#include <algorithm>
#include <numeric>
#include <set>

#include "edit_check_common.h"
#include "lbvh.h"

// ---- the device builder's steps, one loop iteration per lane ----
struct Lbvh {
  std::vector<uint64_t> keys;    // sorted
  std::vector<uint32_t> order;   // sorted file indices
  std::vector<DNode4> sparse;    // indexed by binary node
};

static Lbvh lbvh_on_host(const Tris &tris, uint32_t leaf = BVH_LEAF) {
  const uint32_t n = (uint32_t)tris.size();
  const float *verts = &tris[0].p1.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = 0; t < n; t++) {
    float c[3];
    lbvh_centroid(verts, t, c);
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
  }
  std::vector<uint64_t> keys(n);
  for (uint32_t t = 0; t < n; t++) {
    float c[3];
    lbvh_centroid(verts, t, c);
    keys[t] = lbvh_key(c, lo, hi);
    CHECK(keys[t] < (1ull << 63), "a key of more than 63 bits");
    for (int a = 0; a < 3; a++)
      if (!(hi[a] > lo[a])) CHECK((keys[t] & (0x1249249249249249ull << (2 - a))) == 0, "an axis of zero extent contributes bits");
  }
  Lbvh L;
  L.order.resize(n);
  std::iota(L.order.begin(), L.order.end(), 0u);
  std::stable_sort(L.order.begin(), L.order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  L.keys.resize(n);
  for (uint32_t k = 0; k < n; k++) L.keys[k] = keys[L.order[k]];
  std::vector<LbvhNode> bin(n > 1 ? n - 1 : 0);
  for (uint32_t i = 0; i + 1 < n; i++) bin[i] = lbvh_node(L.keys.data(), n, i);
  L.sparse.resize(n > 1 ? n - 1 : 1);
  for (uint32_t i = 0; i < L.sparse.size(); i++) lbvh_collapse(bin.data(), L.keys.data(), n, leaf, i, L.sparse.data());
  return L;
}

static void check_lbvh(const char *what, const Tris &tris) {
  const uint32_t n = (uint32_t)tris.size();
  const Lbvh L = lbvh_on_host(tris);
  std::vector<DNode4> nodes;
  uint32_t levels = 0;
  const bool ok = lbvh_accept(L.sparse.data(), (uint32_t)L.sparse.size(), L.order.data(), n, BVH_LEAF, nodes, &levels);
  CHECK(ok, "%s: the tree is refused (%u levels)", what, levels);
  if (!ok) return;
  const uint32_t nn = (uint32_t)nodes.size();
  for (uint32_t k = 1; k < n; k++) CHECK(L.keys[k - 1] <= L.keys[k], "%s: keys not sorted", what);
  // every triangle in exactly one leaf of 1 .. BVH_LEAF, every child after its parent, every node reached
  std::vector<int> leaf_of(n, 0), parents(nn, 0);
  for (uint32_t i = 0; i < nn; i++) {
    int used = 0;
    bool gap = false;
    for (int c = 0; c < 4; c++) {
      const uint32_t d = nodes[i].child[c];
      if (d == BVH_LEAF_FLAG) { gap = true; continue; }
      CHECK(!gap, "%s: node %u: a used slot after an unused one", what, i);
      used++;
      if (d & BVH_LEAF_FLAG) {
        const uint32_t first = d & 0xFFFFFFu, count = (d >> 24) & 0x7Fu;
        CHECK(count >= 1 && count <= BVH_LEAF && first + count <= n, "%s: node %u: leaf (%u, %u)", what, i, first, count);
        for (uint32_t k = first; k < first + count && k < n; k++) leaf_of[L.order[k]]++;
      } else {
        CHECK(d > i && d < nn, "%s: node %u: child %u is not a later node", what, i, d);
        if (d < nn) parents[d]++;
      }
    }
    CHECK(used >= (nn == 1 ? 1 : 2) && nodes[i].axis < 3, "%s: node %u: %d used slots, axis %u", what, i, used, nodes[i].axis);
  }
  for (uint32_t t = 0; t < n; t++) CHECK(leaf_of[t] == 1, "%s: triangle %u is in %d leaves", what, t, leaf_of[t]);
  for (uint32_t i = 1; i < nn; i++) CHECK(parents[i] == 1, "%s: node %u has %d parents", what, i, parents[i]);
  LevelSchedule S;
  CHECK(level_schedule(nodes.data(), nn, n, S) && S.levels() == levels, "%s: level_schedule: %zu levels, lbvh_accept %u", what, S.levels(), levels);
  if (n <= BVH_LEAF) CHECK(nn == 1 && levels == 1, "%s: %u nodes, %u levels for one leaf", what, nn, levels);
  // after refit_slot every box is the min / max of what lies below it
  std::vector<DTri> recs(n);
  float gn[4];
  for (uint32_t k = 0; k < n; k++) make_tri(tris[L.order[k]].p1, tris[L.order[k]].p2, tris[L.order[k]].p3, L.order[k], recs[k], gn);
  refit_on_host(nodes.data(), S, recs.data(), tris);
  for (uint32_t i = 0; i < nn; i++)
    for (int c = 0; c < 4; c++) {
      if (nodes[i].child[c] == BVH_LEAF_FLAG) continue;
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      brute(nodes, nodes[i].child[c], L.order, tris, lo, hi);
      for (int a = 0; a < 3; a++) CHECK(nodes[i].lo[a][c] == lo[a] && nodes[i].hi[a][c] == hi[a], "%s: node %u slot %d axis %d: box is not the min / max of what lies below", what, i, c, a);
    }
  float box[6];
  refit_mesh_box(nodes[0], box);
  ctr_vec3 mn, mx;
  ctr_mesh_bounds(tris.data(), tris.size(), &mn, &mx);
  CHECK(box[0] == mn.x && box[1] == mn.y && box[2] == mn.z && box[3] == mx.x && box[4] == mx.y && box[5] == mx.z, "%s: the root's union is not ctr_mesh_bounds", what);
  const MeshTree H = host_mesh_tree(tris.data(), n);
  LevelSchedule SH;
  level_schedule(H.nodes.data(), (uint32_t)H.nodes.size(), n, SH);
  printf("lbvh %-28s triangles %6u nodes %6u levels %2u host_nodes %6zu host_levels %2zu\n", what, n, nn, levels, H.nodes.size(), SH.levels());
}

// 63 tiny triangles, their centroids at 2^-m, m = 0 .. 20, on each coordinate axis of the unit cube: every key has its own highest
// bit, so every split of the radix tree peels ONE key off and the collapsed tree loses two triangles per level
static Tris staircase() {
  Tris t;
  for (int m = 0; m <= 20; m++)
    for (int axis = 0; axis < 3; axis++) {
      float c[3] = {0.f, 0.f, 0.f}, e[3];
      c[axis] = std::ldexp(1.0f, -m);
      for (int a = 0; a < 3; a++) e[a] = c[a] != 0.f ? std::ldexp(c[a], -10) : std::ldexp(1.0f, -30);  // (c - e and c + e are exact: the box's centre is c)
      t.push_back(ctr_triangle{{c[0] - e[0], c[1] - e[1], c[2] - e[2]}, {c[0] + e[0], c[1] + e[1], c[2] + e[2]}, {c[0] + e[0], c[1] - e[1], c[2]}});
    }
  return t;
}

static void check_staircase() {
  const Tris t = staircase();
  const Lbvh L = lbvh_on_host(t);
  std::vector<DNode4> nodes;
  uint32_t levels = 0;
  const bool ok = lbvh_accept(L.sparse.data(), (uint32_t)L.sparse.size(), L.order.data(), (uint32_t)t.size(), BVH_LEAF, nodes, &levels);
  printf("staircase triangles %zu levels %u accepted %d\n", t.size(), levels, (int)ok);
  // the host builder, which the call falls back to, does take them
  const MeshTree H = host_mesh_tree(t.data(), t.size());
  LevelSchedule S;
  CHECK(level_schedule(H.nodes.data(), (uint32_t)H.nodes.size(), (uint32_t)t.size(), S), "staircase: the host's tree has no schedule");
}

static void check_broken() {
  const Tris t = random_tris(40, 2.f, 0.3f);
  const Lbvh L = lbvh_on_host(t);
  const uint32_t n = 40, ns = (uint32_t)L.sparse.size();
  std::vector<DNode4> nodes;
  auto refused = [&](const char *what, const std::vector<DNode4> &sparse, const std::vector<uint32_t> &order) {
    CHECK(!lbvh_accept(sparse.data(), (uint32_t)sparse.size(), order.data(), n, BVH_LEAF, nodes), "broken: %s is accepted", what);
  };
  CHECK(lbvh_accept(L.sparse.data(), ns, L.order.data(), n, BVH_LEAF, nodes), "broken: the unbroken tree is refused");
  uint32_t inner = 0xFFFFFFFFu, leaf_node = 0, leaf_slot = 0;  // an inner child of the root; some leaf slot
  for (int c = 0; c < 4; c++)
    if (!(L.sparse[0].child[c] & BVH_LEAF_FLAG)) inner = L.sparse[0].child[c];
  CHECK(inner != 0xFFFFFFFFu, "broken: the root of 40 triangles has an inner child");
  for (bool found = false; !found;) {  // a leaf slot of a node the root reaches: down the first inner child until one shows
    uint32_t next = leaf_node;
    for (int c = 3; c >= 0; c--) {
      const uint32_t d = L.sparse[leaf_node].child[c];
      if (d != BVH_LEAF_FLAG && (d & BVH_LEAF_FLAG)) { leaf_slot = (uint32_t)c; found = true; }
      else if (d != BVH_LEAF_FLAG) next = d;
    }
    if (!found) leaf_node = next;
  }
  std::vector<DNode4> s;
  s = L.sparse; s[inner].child[0] = 0u; refused("a cycle through the root", s, L.order);
  s = L.sparse; s[inner].child[0] = inner; refused("a node that is its own child", s, L.order);
  s = L.sparse; s[0].child[3] = s[0].child[0]; refused("a child shared by two slots", s, L.order);
  s = L.sparse; s[0].child[0] = ns + 7u; refused("a child index past the array", s, L.order);
  s = L.sparse; s[leaf_node].child[leaf_slot] = BVH_LEAF_FLAG; refused("an uncovered triangle", s, L.order);
  s = L.sparse; s[leaf_node].child[leaf_slot] = BVH_LEAF_FLAG | (4u << 24) | (n - 2u); refused("a leaf past the mesh", s, L.order);
  s = L.sparse; s[leaf_node].child[leaf_slot] = BVH_LEAF_FLAG | (5u << 24) | (s[leaf_node].child[leaf_slot] & 0xFFFFFFu); refused("a leaf of five", s, L.order);
  std::vector<uint32_t> o = L.order;
  o[3] = o[4]; refused("an order with a triangle twice", L.sparse, o);
  o = L.order; o[0] = n; refused("an order with an index past the mesh", L.sparse, o);
  printf("broken trees refused\n");
}

// ---- install: the scenes of mesh_update_check.cpp ----
static const float EYE[3] = {0.3f, 0.2f, 0.5f};

static Scene scene_of(const Tris &a, const Tris &b) {
  Scene s;
  ctr_material m{};
  m.type = CTR_MAT_PHONG;
  m.color = ctr_vec3{0.5f, 0.5f, 0.5f};
  s.materials.push_back(m);
  m.reflexivity = 0.5f;
  s.materials.push_back(m);
  s.lights.push_back(light(CTR_LIGHT_POINT, 5.f, 6.f, 7.03f));
  s.mesh(a, 0);
  s.plane(ctr_vec3{0, -9, 0}, ctr_vec3{0, 1, 0}, 0);
  if (!b.empty()) s.mesh(b, 1);
  s.cam.pos = ctr_vec3{EYE[0], EYE[1], EYE[2]};
  s.cam.w = s.cam.h = 16;
  s.finish();
  return s;
}

// ctr_scene_rebuild_mesh on the host copy: mesh_rebuilt, then the update's steps
static bool rebuild_on_host(FlatScene &F, size_t gi, const MeshTree &tree, const Tris &nt) {
  bool was_moved = false;
  mesh_rebuilt(F, gi, tree, &was_moved);
  update_on_host(F, gi, nt);
  return was_moved;
}

// the LBVH text's tree over `t`, accepted
static MeshTree lbvh_tree(const Tris &t) {
  const Lbvh L = lbvh_on_host(t);
  MeshTree tree;
  tree.order = L.order;
  CHECK(lbvh_accept(L.sparse.data(), (uint32_t)L.sparse.size(), L.order.data(), (uint32_t)t.size(), BVH_LEAF, tree.nodes), "install: the LBVH tree is refused");
  return tree;
}

// mesh gi of A (rebuilt) against mesh gi of B (fresh), relative to their ranges: per FILE triangle the same record, normal and
// plane; the same box wherever it is kept; the guard picks the same FILE triangles; the records name A's range; every box of
// A's tree holds what lies below it
static void same_mesh(const char *what, const FlatScene &A, const FlatScene &B, size_t gi, const Tris &nt) {
  const MeshGuard &ga = A.guards[gi], &gb = B.guards[gi];
  CHECK(ga.tri_count == gb.tri_count && ga.tri_begin == gb.tri_begin, "%s: triangle range", what);
  std::vector<uint32_t> at_b(gb.tri_count), order_a(ga.tri_count);
  for (uint32_t k = 0; k < gb.tri_count; k++) at_b[B.tris[gb.tri_begin + k].orig] = k;
  size_t bad = 0;
  for (uint32_t k = 0; k < ga.tri_count; k++) {
    const uint32_t f = A.tris[ga.tri_begin + k].orig, kb = at_b[f];
    order_a[k] = f;
    bad += memcmp(&A.tris[ga.tri_begin + k], &B.tris[gb.tri_begin + kb], sizeof(DTri)) != 0;
    bad += memcmp(&A.gn[4 * (ga.tri_begin + f)], &B.gn[4 * (gb.tri_begin + f)], 16) != 0;
    bad += memcmp(&ga.planes[CTR_PLANE_DOUBLES * k], &gb.planes[CTR_PLANE_DOUBLES * kb], CTR_PLANE_DOUBLES * sizeof(double)) != 0;
  }
  CHECK(bad == 0, "%s: %zu records, normals or planes differ from the fresh scene's", what, bad);
  auto names_range = [&](const DObj &O) { return O.node_begin == ga.node_begin && O.node_count == ga.node_count && O.bvh_root == (ga.guarded.empty() ? 0u : ga.node_count); };
  CHECK(names_range(A.objs[ga.obj_index]) && names_range(A.meshes[ga.mesh_pos]), "%s: objs / meshes do not name the mesh's node range", what);
  for (int q = 0; q < 6; q++) {
    CHECK(A.objs[ga.obj_index].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in objs", what, q);
    CHECK(A.meshes[ga.mesh_pos].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in meshes", what, q);
  }
  for (size_t k = A.n_mesh + 1; k < A.meshes.size(); k++)
    if (A.meshes[k].index == ga.obj_index) {
      CHECK(A.meshes[k].node_begin == ga.node_begin && A.meshes[k].node_count == ga.node_count, "%s: the scene-order copy does not name the range", what);
      for (int q = 0; q < 6; q++) CHECK(A.meshes[k].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in the scene-order copy", what, q);
    }
  for (int a = 0; a < 3; a++) CHECK(A.tl_mn[a] == B.tl_mn[a] && A.tl_mx[a] == B.tl_mx[a], "%s: tl_mn / tl_mx", what);
  std::set<uint32_t> fa, fb;
  for (uint32_t t : ga.guarded) fa.insert(A.tris[ga.tri_begin + t].orig);
  for (uint32_t t : gb.guarded) fb.insert(B.tris[gb.tri_begin + t].orig);
  CHECK(fa == fb && ga.linear == gb.linear, "%s: guarded %zu / %zu triangles, linear %d / %d", what, fa.size(), fb.size(), (int)ga.linear, (int)gb.linear);
  // the installed tree, relative to its range
  CHECK((size_t)ga.node_begin + ga.node_cap + 1u <= A.nodes4.size() && ga.node_count <= ga.node_cap, "%s: the node range leaves the array", what);
  const std::vector<DNode4> nodes(A.nodes4.begin() + ga.node_begin, A.nodes4.begin() + ga.node_begin + ga.node_count);
  LevelSchedule S;
  CHECK(level_schedule(nodes.data(), ga.node_count, ga.tri_count, S), "%s: no schedule for the installed tree", what);
  for (uint32_t i = 0; i < ga.node_count; i++)
    for (int c = 0; c < 4; c++) {
      if (nodes[i].child[c] == BVH_LEAF_FLAG) continue;
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      brute(nodes, nodes[i].child[c], order_a, nt, lo, hi);
      for (int a = 0; a < 3; a++) CHECK(nodes[i].lo[a][c] == lo[a] && nodes[i].hi[a][c] == hi[a], "%s: node %u slot %d: host copy's box", what, i, c);
    }
  const DNode4 empty = empty_node4();
  for (uint32_t k = ga.node_count + 1u; k <= ga.node_cap; k++) CHECK(!memcmp(&A.nodes4[ga.node_begin + k], &empty, sizeof(empty)), "%s: unused node %u of the range is not empty", what, k);
  CHECK(A.ray_slots == ray_stack_slots(A), "%s: ray_slots %u, of the trees %u", what, A.ray_slots, ray_stack_slots(A));
  CHECK(A.mesh_bytes == A.tris.size() * sizeof(DTri) + A.nodes.size() * sizeof(DNode) + A.nodes4.size() * sizeof(DNode4), "%s: mesh_bytes", what);
  printf("rebuild %-44s guarded %2zu linear %d nodes %4u\n", what, fa.size(), (int)ga.linear, ga.node_count);
}

static void check_install() {
  Tris a = random_tris(150, 1.5f, 0.3f), b = random_tris(12, 0.5f, 0.4f);
  for (ctr_triangle &t : a) { t.p1.z += 3.f; t.p2.z += 3.f; t.p3.z += 3.f; }  // (off the plane z = 0.5)
  a.push_back(ctr_triangle{{0.1f, 0.1f, 2.f}, {0.1f, 0.1f, 2.f}, {0.1f, 0.1f, 2.f}});  // zero area: a point, three points of a line
  a.push_back(ctr_triangle{{0, 0, 2.f}, {0.5f, 0.5f, 2.f}, {1, 1, 2.f}});

  // ---- bvh4_build's own tree over the same triangles: in place, byte for byte the fresh scene (one mesh: no merged tree to retire) ----
  {
    const Scene s = scene_of(a, Tris());
    FlatScene A = flat_of(s.desc), B = flat_of(s.desc);
    guard(A, EYE);
    guard(B, EYE);
    const size_t nodes_before = A.nodes4.size();
    const bool mv = rebuild_on_host(A, 0, host_mesh_tree(a.data(), a.size()), a);
    guard(A, EYE);
    CHECK(!mv && A.nodes4.size() == nodes_before, "in place: the builder's own tree moved");
    same_flat("in place, the builder's own tree", A, B);
    printf("install in place: moved %d\n", (int)mv);
    // ... and with moved triangles through the LBVH text: whatever its node count, the mesh is the fresh scene's
    const Tris am = moved(a, 0.8f, 0.1f);
    const MeshTree T = lbvh_tree(am);
    const bool mv2 = rebuild_on_host(A, 0, T, am);
    guard(A, EYE);
    const Scene s2 = scene_of(am, Tris());
    FlatScene B2 = flat_of(s2.desc);
    guard(B2, EYE);
    CHECK(mv2 == (T.nodes.size() > B.guards[0].node_count), "lbvh: moved %d with %zu nodes for a range of %u", (int)mv2, T.nodes.size(), B.guards[0].node_count);
    same_mesh("one mesh, LBVH tree", A, B2, 0, am);
  }

  // ---- two meshes; leaf size 1: more nodes than the range holds, the mesh moves ----
  const Scene s0 = scene_of(a, b);
  FlatScene A = flat_of(s0.desc);
  guard(A, EYE);
  CHECK(!build_merged_tree(A).empty() && A.merged.built, "the merged tree of two meshes builds");
  guard(A, EYE);
  {
    const FlatScene before = A;
    const MeshTree T1 = host_mesh_tree(a.data(), a.size(), 1);
    CHECK(T1.nodes.size() > before.guards[0].node_count, "leaf size 1 gives %zu nodes, no more than %u", T1.nodes.size(), before.guards[0].node_count);
    const bool mv = rebuild_on_host(A, 0, T1, a);
    guard(A, EYE);
    const MeshGuard &g = A.guards[0], &o = A.guards[1], &o0 = before.guards[1];
    CHECK(mv && g.node_begin == before.nodes4.size() && g.node_count == T1.nodes.size() && g.node_cap == g.node_count &&
          A.nodes4.size() == before.nodes4.size() + T1.nodes.size() + 1u, "moved: range (%u, %u) in an array of %zu, before %zu", g.node_begin, g.node_count, A.nodes4.size(), before.nodes4.size());
    CHECK(!A.merged.reserved && !A.merged.built && !A.merged.usable, "moved: the merged tree is retired");
    // the other mesh: its records, triangles, normals, planes and nodes are untouched
    CHECK(o.node_begin == o0.node_begin && o.node_count == o0.node_count && o.tri_begin == o0.tri_begin && o.guarded == o0.guarded && o.linear == o0.linear, "moved: the other mesh's guard record");
    CHECK(!memcmp(&A.objs[o.obj_index], &before.objs[o.obj_index], sizeof(DObj)) && !memcmp(&A.meshes[o.mesh_pos], &before.meshes[o.mesh_pos], sizeof(DObj)), "moved: the other mesh's records");
    CHECK(!memcmp(&A.tris[o.tri_begin], &before.tris[o.tri_begin], (o.tri_count + CTR_GUARD_SLOTS) * sizeof(DTri)) &&
          !memcmp(&A.gn[4 * (size_t)o.tri_begin], &before.gn[4 * (size_t)o.tri_begin], (o.tri_count + CTR_GUARD_SLOTS) * 16) && same_bytes(o.planes, o0.planes), "moved: the other mesh's triangles");
    CHECK(!memcmp(&A.nodes4[o.node_begin], &before.nodes4[o.node_begin], (o.node_count + 1u) * sizeof(DNode4)), "moved: the other mesh's nodes");
    for (uint32_t i = 0; i < g.node_count; i++)
      CHECK(!memcmp(A.nodes4[g.node_begin + i].child, T1.nodes[i].child, 16) && A.nodes4[g.node_begin + i].axis == T1.nodes[i].axis, "moved: node %u is not the builder's", i);
    FlatScene B = flat_of(s0.desc);
    guard(B, EYE);
    same_mesh("two meshes, leaf size 1: moved", A, B, 0, a);
    printf("install leaf size 1: moved %d nodes %u range %u\n", (int)mv, g.node_count, before.guards[0].node_count);
    // a smaller tree afterwards fits the new range: in place again
    const bool mv2 = rebuild_on_host(A, 0, host_mesh_tree(a.data(), a.size()), a);
    guard(A, EYE);
    CHECK(!mv2 && A.guards[0].node_begin == g.node_begin && A.guards[0].node_cap == T1.nodes.size(), "a smaller tree after the move moved again");
    same_mesh("two meshes, back to leaf size 4: in place", A, B, 0, a);
  }

  // ---- the in-plane cases of mesh_update_check.cpp through rebuilds with the LBVH text's tree ----
  struct Step { const char *what; Tris tris; bool linear; } steps[] = {
      {"moved", moved(a, 0.5f, 0.02f), false}, {"3 in the eye's plane", with_in_plane(a, 3), false}, {"70 in the eye's plane", with_in_plane(a, 70), true},
      {"70 again: linear payload after refit", with_in_plane(moved(a, 0.1f, 0.0f), 70), true}, {"none in the plane", moved(a, -0.3f, 0.01f), false}};
  for (const Step &st : steps) {
    rebuild_on_host(A, 0, lbvh_tree(st.tris), st.tris);
    const std::vector<DirtyRange> dirty = guard(A, EYE);
    bool payload = false;
    for (const DirtyRange &r : dirty)
      if (r.array == DirtyRange::NODES4 && r.begin == A.guards[0].node_begin && !r.payload.empty()) {
        payload = true;
        CHECK(r.count == A.guards[0].node_count && r.payload.size() == r.count, "%s: payload of %zu nodes for a tree of %u", st.what, r.payload.size(), A.guards[0].node_count);
        for (const DNode4 &N : r.payload)
          for (int c = 0; c < 4; c++)
            if (N.child[c] != BVH_LEAF_FLAG) CHECK(N.lo[0][c] == -3.0e38f && N.hi[2][c] == 3.0e38f, "%s: payload slot not unbounded", st.what);
      }
    CHECK(payload == st.linear, "%s: unbounded payload %s", st.what, payload ? "sent" : "not sent");
    CHECK(guard(A, EYE).empty(), "%s: the same cameras again change nothing", st.what);
    const Scene s1 = scene_of(st.tris, b);
    FlatScene B = flat_of(s1.desc);
    guard(B, EYE);
    same_mesh(st.what, A, B, 0, st.tris);
  }
  // ---- the reflective 12-triangle mesh rebuilt: its triangles are mirrors, the virtual eyes follow ----
  const Tris b2 = moved(b, 1.0f, 0.0f);
  rebuild_on_host(A, 1, lbvh_tree(b2), b2);
  guard(A, EYE);
  const Scene s2 = scene_of(steps[4].tris, b2);
  FlatScene B = flat_of(s2.desc);
  guard(B, EYE);
  same_mesh("reflective mesh rebuilt", A, B, 1, b2);
  same_mesh("reflective mesh rebuilt: the other mesh", A, B, 0, steps[4].tris);
}

int main() {
  auto flat_set = [](size_t n) { Tris t = random_tris(n, 5.f, 0.4f); for (ctr_triangle &q : t) q.p1.x = q.p2.x = q.p3.x = 1.25f; return t; };
  auto line_set = [](size_t n) {  // all centroids on the line x = y = z
    Tris t(n);
    for (ctr_triangle &q : t) {
      const float c = U(-3.f, 3.f), e = 0.125f;
      q = ctr_triangle{{c - e, c - e, c - e}, {c + e, c + e, c + e}, {c + e, c - e, c}};
    }
    return t;
  };
  // Triangle positions and sizes over ten octaves.  A key spends three bits per octave, so the radix tree is about thirty splits
  // deep where the cluster is densest and the collapsed tree half of that: deeper than the host's, inside what the walk's stack
  // holds.  (Over mesh_update_check.cpp's 120 octaves the keys peel off like the staircase's and the tree is refused.)
  auto cluster = [](size_t n) {
    Tris t = random_tris(n, 1.f, 0.01f);
    for (size_t i = 0; i < t.size(); i++) {
      const float s = std::ldexp(1.0f, -(int)(i % 10));
      for (int j = 0; j < 9; j++) (&t[i].p1.x)[j] *= s;
    }
    return t;
  };
  for (size_t n : {1u, 2u, 4u, 5u, 64u, 65u, 1000u, 20000u}) check_lbvh(("random " + std::to_string(n)).c_str(), random_tris(n, 10.f, 0.5f));
  check_lbvh("70 identical triangles", Tris(70, ctr_triangle{{1, 2, 3}, {2, 2, 3}, {1, 3, 3}}));
  check_lbvh("flat in x", flat_set(2000));
  check_lbvh("centroids on a line", line_set(500));
  check_lbvh("geometric cluster", cluster(5000));
  check_lbvh("geometric cluster of 200", cluster(200));
  check_staircase();
  check_broken();
  check_install();
  printf(fails ? "mesh_rebuild_check: %d FAILURES\n" : "mesh_rebuild_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
