// mesh_replace_check.cpp — the host-checkable half of ctr_scene_replace_mesh (include/cutrace_replace.h) without a device; meant to run
// under ASan/UBSan as well.  tests/test_mesh_replace_cpu.py builds and runs it and reads the lines it prints.
//
// A flattened scene goes through replaces — mesh_replaced (scene_flatten.cpp) with the update's steps behind it (update_on_host), then
// the guard — and each result is compared with flatten_scene of the replaced description.  The replaced scene's ranges lie elsewhere,
// so the comparison is relative to them: per mesh its triangle records, normals, guard planes, guard records, nodes (child
// descriptors are relative to the mesh's first node and first triangle) and box; the top-level tree; ray_slots, mesh_tris and
// mesh_bytes of the live records; every array that holds no mesh data byte for byte.  With the host's builder at its default leaf
// size the tree is the fresh scene's own and the nodes agree byte for byte; a tree of another shape (leaf size 1 or 2) is checked
// box by box against the triangles below it.
#include <set>

#include "edit_check_common.h"

static const float EYE[3] = {0.3f, 0.2f, 0.5f};

// off the plane z = 0.5 that holds the eye
static Tris lifted(Tris t, float dz = 3.f) {
  for (ctr_triangle &q : t) { q.p1.z += dz; q.p2.z += dz; q.p3.z += dz; }
  return t;
}

// ... and far along x: whatever the two meshes of a scene become, the top-level builder splits them along x, the first mesh first, so
// that the top-level tree of the replaced scene, which keeps its shape, can be compared with the fresh scene's byte for byte
static Tris aside(Tris t, float dx = 20.f) {
  for (ctr_triangle &q : t) { q.p1.x += dx; q.p2.x += dx; q.p3.x += dx; }
  return t;
}

// scene_of(a) / scene_of(a, b) of mesh_rebuild_check.cpp: mesh a (material 0), a floor, mesh b (reflecting material 1); or, mixed:
// mesh a, a stand-alone triangle, mesh b, a sphere, in that order
static Scene scene_of(const Tris &a, const Tris &b, bool mixed = false) {
  Scene s;
  ctr_material m{};
  m.type = CTR_MAT_PHONG;
  m.color = ctr_vec3{0.5f, 0.5f, 0.5f};
  s.materials.push_back(m);
  m.reflexivity = 0.5f;
  s.materials.push_back(m);
  s.lights.push_back(light(CTR_LIGHT_POINT, 5.f, 6.f, 7.03f));
  s.mesh(a, 0);
  if (mixed) s.triangle(ctr_vec3{-4.f, 1.f, 2.f}, ctr_vec3{-3.f, 1.5f, 2.5f}, ctr_vec3{-3.5f, 2.f, 1.f}, 0);
  else s.plane(ctr_vec3{0, -9, 0}, ctr_vec3{0, 1, 0}, 0);
  if (!b.empty()) s.mesh(b, mixed ? 0 : 1);
  if (mixed) s.sphere(ctr_vec3{4.f, 0.f, 3.f}, 0.7f, 0);
  s.cam.pos = ctr_vec3{EYE[0], EYE[1], EYE[2]};
  s.cam.w = s.cam.h = 16;
  s.finish();
  return s;
}

struct Moves { bool tris, nodes; };

// ctr_scene_replace_mesh on the host copy: mesh_replaced, then the update's steps, then the guard
static Moves replace_on_host(FlatScene &F, size_t gi, const Tris &nt, uint32_t leaf = BVH_LEAF) {
  Moves mv{false, false};
  const ReplaceRoom room = replace_room(F, gi, (uint32_t)nt.size(), (uint32_t)host_mesh_tree(nt.data(), nt.size(), leaf).nodes.size());
  const size_t tris_before = F.tris.size(), nodes_before = F.nodes4.size();
  const MeshTree tree = host_mesh_tree(nt.data(), nt.size(), leaf);
  mesh_replaced(F, gi, (uint32_t)nt.size(), tree, &mv.tris, &mv.nodes);
  CHECK(mv.tris == room.tris_move && mv.nodes == room.nodes_move && F.tris.size() == room.tris_after && F.gn.size() == 4 * room.tris_after &&
        F.nodes4.size() == room.nodes4_after && F.guards[gi].tri_cap == room.tri_cap && F.guards[gi].node_cap == room.node_cap,
        "replace_room does not say what mesh_replaced did");
  CHECK(F.tris.size() == tris_before + (mv.tris ? (size_t)room.tri_cap + CTR_GUARD_SLOTS : 0u) && F.nodes4.size() == nodes_before + (mv.nodes ? (size_t)room.node_cap + 1u : 0u),
        "the arrays grew by something other than the new ranges");
  update_on_host(F, gi, nt);
  guard(F, EYE);
  return mv;
}

// the live ranges of A: inside their arrays, and no two of them share a record
static void ranges_are_disjoint(const char *what, const FlatScene &A) {
  std::vector<std::pair<size_t, size_t>> tr, nd;
  for (const DObj &O : A.objs)
    if (O.type == CTR_OBJ_TRIANGLE) tr.push_back({O.tri_begin, O.tri_begin + 1u});
  for (const MeshGuard &g : A.guards) {
    if (g.tri_count) tr.push_back({g.tri_begin, (size_t)g.tri_begin + g.tri_cap + CTR_GUARD_SLOTS});
    nd.push_back({g.node_begin, (size_t)g.node_begin + g.node_cap + 1u});
    CHECK(g.tri_count <= g.tri_cap && g.node_count <= g.node_cap, "%s: a count above its room", what);
  }
  if (A.merged.tri_count) {  // the merged tree's room, reserved or retired
    tr.push_back({A.merged.tri_begin, (size_t)A.merged.tri_begin + A.merged.tri_count + CTR_GUARD_SLOTS});
    nd.push_back({A.merged.node_begin, (size_t)A.merged.node_begin + A.merged.node_cap + CTR_MERGED_SPARE_NODES});
  }
  auto disjoint = [&](std::vector<std::pair<size_t, size_t>> &r, size_t size, const char *name) {
    std::sort(r.begin(), r.end());
    for (size_t k = 0; k < r.size(); k++) {
      CHECK(r[k].second <= size, "%s: a %s range ends at %zu in an array of %zu", what, name, r[k].second, size);
      if (k) CHECK(r[k - 1].second <= r[k].first, "%s: two %s ranges overlap at %zu", what, name, r[k].first);
    }
  };
  disjoint(tr, A.tris.size(), "triangle");
  disjoint(nd, A.nodes4.size(), "node");
  CHECK(A.gn.size() == 4 * A.tris.size(), "%s: gn has %zu floats for %zu records", what, A.gn.size(), A.tris.size());
}

// mesh gi of A (replaced) against mesh gi of B (fresh), relative to their ranges.  same_tree: A's tree came from the builder B's came
// from, and nodes, leaf order and guard records agree byte for byte; otherwise the tree is checked against the triangles
static void same_mesh(const char *what, const FlatScene &A, const FlatScene &B, size_t gi, const Tris &nt, bool same_tree) {
  const MeshGuard &ga = A.guards[gi], &gb = B.guards[gi];
  CHECK(ga.tri_count == gb.tri_count && ga.tri_count == nt.size() && ga.obj_index == gb.obj_index && ga.mesh_pos == gb.mesh_pos, "%s: mesh %zu: count %u / %u", what, gi, ga.tri_count, gb.tri_count);
  if (ga.tri_count != gb.tri_count) return;
  CHECK(ga.planes.size() == (size_t)CTR_PLANE_DOUBLES * ga.tri_count, "%s: mesh %zu: %zu plane doubles", what, gi, ga.planes.size());
  std::vector<uint32_t> at_b(gb.tri_count), order_a(ga.tri_count);
  for (uint32_t k = 0; k < gb.tri_count; k++) at_b[B.tris[gb.tri_begin + k].orig] = k;
  size_t bad = 0;
  for (uint32_t k = 0; k < ga.tri_count; k++) {
    const uint32_t f = A.tris[ga.tri_begin + k].orig;
    CHECK(f < ga.tri_count, "%s: mesh %zu: record %u names triangle %u", what, gi, k, f);
    if (f >= ga.tri_count) return;
    const uint32_t kb = at_b[f];
    order_a[k] = f;
    if (same_tree) bad += kb != k;
    bad += memcmp(&A.tris[ga.tri_begin + k], &B.tris[gb.tri_begin + kb], sizeof(DTri)) != 0;
    bad += memcmp(&A.gn[4 * ((size_t)ga.tri_begin + f)], &B.gn[4 * ((size_t)gb.tri_begin + f)], 16) != 0;  // gn: FILE index inside the range
    bad += memcmp(&ga.planes[CTR_PLANE_DOUBLES * k], &gb.planes[CTR_PLANE_DOUBLES * kb], CTR_PLANE_DOUBLES * sizeof(double)) != 0;
  }
  CHECK(bad == 0, "%s: mesh %zu: %zu records, normals or planes differ from the fresh scene's", what, gi, bad);
  // the guard: the same FILE triangles, the same state; the records behind the new count
  std::set<uint32_t> fa, fb;
  for (uint32_t t : ga.guarded) fa.insert(A.tris[ga.tri_begin + t].orig);
  for (uint32_t t : gb.guarded) fb.insert(B.tris[gb.tri_begin + t].orig);
  CHECK(fa == fb && ga.linear == gb.linear, "%s: mesh %zu: guarded %zu / %zu triangles, linear %d / %d", what, gi, fa.size(), fb.size(), (int)ga.linear, (int)gb.linear);
  for (size_t k = 0; k < ga.guarded.size(); k++)
    CHECK(!memcmp(&A.tris[ga.tri_begin + ga.tri_count + k], &A.tris[ga.tri_begin + ga.guarded[k]], sizeof(DTri)), "%s: mesh %zu: guard record %zu is not its triangle", what, gi, k);
  if (same_tree)
    CHECK(!memcmp(&A.tris[ga.tri_begin + ga.tri_count], &B.tris[gb.tri_begin + gb.tri_count], CTR_GUARD_SLOTS * sizeof(DTri)) &&
          !memcmp(&A.gn[4 * ((size_t)ga.tri_begin + ga.tri_count)], &B.gn[4 * ((size_t)gb.tri_begin + gb.tri_count)], CTR_GUARD_SLOTS * 16), "%s: mesh %zu: the spare records", what, gi);
  // the records of the mesh: equal but for where the ranges begin
  auto same_record = [&](DObj a, DObj b) {
    CHECK(a.tri_begin == ga.tri_begin && a.node_begin == ga.node_begin && b.tri_begin == gb.tri_begin && b.node_begin == gb.node_begin, "%s: mesh %zu: a record does not name the mesh's ranges", what, gi);
    a.tri_begin = b.tri_begin = a.node_begin = b.node_begin = 0;
    if (!same_tree) {
      CHECK(a.node_count == ga.node_count && a.bvh_root == (ga.guarded.empty() ? 0u : ga.node_count), "%s: mesh %zu: node_count / bvh_root of a record", what, gi);
      a.node_count = b.node_count = a.bvh_root = b.bvh_root = 0;
    }
    return !memcmp(&a, &b, sizeof(DObj));
  };
  CHECK(same_record(A.objs[ga.obj_index], B.objs[gb.obj_index]), "%s: mesh %zu: objs", what, gi);
  CHECK(same_record(A.meshes[ga.mesh_pos], B.meshes[gb.mesh_pos]), "%s: mesh %zu: meshes", what, gi);
  for (size_t k = A.n_mesh + 1; k < A.meshes.size(); k++)
    if (A.meshes[k].index == ga.obj_index) {
      CHECK(A.meshes[k].tri_begin == ga.tri_begin && A.meshes[k].tri_count == ga.tri_count && A.meshes[k].node_begin == ga.node_begin && A.meshes[k].node_count == ga.node_count,
            "%s: mesh %zu: the scene-order copy does not name the ranges", what, gi);
      for (int q = 0; q < 6; q++) CHECK(A.meshes[k].f[q] == B.objs[gb.obj_index].f[q], "%s: mesh %zu: box word %d in the scene-order copy", what, gi, q);
    }
  // the tree, relative to its range
  const std::vector<DNode4> nodes(A.nodes4.begin() + ga.node_begin, A.nodes4.begin() + ga.node_begin + ga.node_count);
  if (same_tree) {
    CHECK(ga.node_count == gb.node_count && !memcmp(nodes.data(), &B.nodes4[gb.node_begin], ga.node_count * sizeof(DNode4)), "%s: mesh %zu: the nodes are not the fresh scene's", what, gi);
    CHECK(!memcmp(&A.nodes4[ga.node_begin + ga.node_count], &B.nodes4[gb.node_begin + gb.node_count], sizeof(DNode4)), "%s: mesh %zu: the spare node", what, gi);
  }
  LevelSchedule S;
  CHECK(level_schedule(nodes.data(), ga.node_count, ga.tri_count, S), "%s: mesh %zu: no schedule for the installed tree", what, gi);
  for (uint32_t i = 0; i < ga.node_count; i++)
    for (int c = 0; c < 4; c++) {
      if (nodes[i].child[c] == BVH_LEAF_FLAG) continue;
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      brute(nodes, nodes[i].child[c], order_a, nt, lo, hi);
      for (int a = 0; a < 3; a++) CHECK(nodes[i].lo[a][c] == lo[a] && nodes[i].hi[a][c] == hi[a], "%s: mesh %zu: node %u slot %d: host copy's box", what, gi, i, c);
    }
  const DNode4 empty = empty_node4();
  for (uint32_t k = ga.node_count + 1u; k <= ga.node_cap; k++) CHECK(!memcmp(&A.nodes4[ga.node_begin + k], &empty, sizeof(empty)), "%s: mesh %zu: unused node %u of the range is not empty", what, gi, k);
}

// A (replaced) against B (fresh), both guarded: every mesh (tris[gi]: its triangles now), and everything that holds no mesh data
static void same_scene(const char *what, const FlatScene &A, const FlatScene &B, const std::vector<Tris> &tris, bool same_tree = true, bool live_bytes = true) {
  ranges_are_disjoint(what, A);
  CHECK(A.guards.size() == B.guards.size() && A.guards.size() == tris.size(), "%s: %zu / %zu meshes", what, A.guards.size(), B.guards.size());
  for (size_t gi = 0; gi < A.guards.size() && gi < B.guards.size(); gi++) same_mesh(what, A, B, gi, tris[gi], same_tree);
  // no mesh data: byte for byte
  CHECK(same_bytes(A.planes, B.planes) && same_bytes(A.lights, B.lights) && same_bytes(A.mats, B.mats) && A.oloop.size() == B.oloop.size(), "%s: planes, lights, mats or the size of oloop", what);
  for (size_t i = 0; i < A.oloop.size() && i < B.oloop.size(); i++) {  // (a stand-alone triangle's copy names its record, which lies behind the first mesh's ORIGINAL range)
    DObj a = A.oloop[i], b = B.oloop[i];
    CHECK(a.index < A.objs.size() && a.tri_begin == A.objs[a.index].tri_begin, "%s: oloop %zu does not name its object's record", what, i);
    a.tri_begin = b.tri_begin = 0;
    CHECK(!memcmp(&a, &b, sizeof(DObj)), "%s: oloop %zu", what, i);
  }
  CHECK(A.objs.size() == B.objs.size(), "%s: objs", what);
  for (size_t i = 0; i < A.objs.size() && i < B.objs.size(); i++) {
    if (A.objs[i].type == CTR_OBJ_MESH) continue;
    DObj a = A.objs[i], b = B.objs[i];
    if (a.type == CTR_OBJ_TRIANGLE) {
      CHECK(!memcmp(&A.tris[a.tri_begin], &B.tris[b.tri_begin], sizeof(DTri)) && !memcmp(&A.gn[4 * (size_t)a.tri_begin], &B.gn[4 * (size_t)b.tri_begin], 16), "%s: the stand-alone triangle's record", what);
      a.tri_begin = b.tri_begin = 0;
    }
    CHECK(!memcmp(&a, &b, sizeof(DObj)), "%s: object %zu", what, i);
  }
  CHECK(A.all_opaque == B.all_opaque && A.need_cold == B.need_cold && A.any_bounce == B.any_bounce && A.fast_pow_ok == B.fast_pow_ok && A.has_mesh == B.has_mesh && A.n_axis_recs == B.n_axis_recs,
        "%s: flags", what);
  // the top-level tree
  CHECK(same_bytes(A.nodes, B.nodes) && A.n_mesh == B.n_mesh && A.tlas_root == B.tlas_root && A.tlas_begin == B.tlas_begin && !memcmp(A.tl_mn, B.tl_mn, 12) && !memcmp(A.tl_mx, B.tl_mx, 12),
        "%s: the top-level tree", what);
  for (size_t k = 0; k < A.n_mesh && k < B.n_mesh; k++) CHECK(A.meshes[k].index == B.meshes[k].index, "%s: top-level leaf %zu holds another mesh", what, k);
  CHECK(!A.merged.reserved && !A.merged.built && !A.merged.usable, "%s: the merged tree is not retired", what);
  // the scalars
  CHECK(A.mesh_tris == B.mesh_tris, "%s: mesh_tris %llu / %llu", what, (unsigned long long)A.mesh_tris, (unsigned long long)B.mesh_tris);
  CHECK(A.ray_slots == ray_stack_slots(A) && (!same_tree || A.ray_slots == B.ray_slots), "%s: ray_slots %u, of the trees %u, fresh %u", what, A.ray_slots, ray_stack_slots(A), B.ray_slots);
  size_t live_t = 0, live_n = 0;
  for (const DObj &O : A.objs) live_t += O.type == CTR_OBJ_TRIANGLE;
  for (const MeshGuard &g : A.guards) { live_t += g.tri_count + (g.tri_count ? CTR_GUARD_SLOTS : 0u); live_n += g.node_count + 1u; }
  if (live_bytes) CHECK(A.mesh_bytes == live_t * sizeof(DTri) + A.nodes.size() * sizeof(DNode) + live_n * sizeof(DNode4), "%s: mesh_bytes is not that of the live records", what);
  // ... which a fresh scene holds and nothing else, but for the room of a merged tree
  const size_t merged_room = B.merged.reserved ? ((size_t)B.merged.tri_count + CTR_GUARD_SLOTS) * sizeof(DTri) + ((size_t)B.merged.node_cap + CTR_MERGED_SPARE_NODES) * sizeof(DNode4) : 0u;
  if (same_tree && live_bytes) CHECK(A.mesh_bytes == B.mesh_bytes - merged_room, "%s: mesh_bytes %zu, the fresh scene's live records %zu", what, A.mesh_bytes, B.mesh_bytes - merged_room);
}

static FlatScene guarded(const Scene &s) {
  FlatScene F = flat_of(s.desc);
  guard(F, EYE);
  return F;
}

static void line(const char *what, const FlatScene &A, size_t gi, Moves mv) {
  const MeshGuard &g = A.guards[gi];
  printf("replace %-40s count %5u tri_cap %5u tris_moved %d nodes_moved %d guarded %2zu linear %d\n", what, g.tri_count, g.tri_cap, (int)mv.tris, (int)mv.nodes, g.guarded.size(), (int)g.linear);
}

// ---- 1, 2, 3, 7: one mesh through a row of counts ----
static void check_counts() {
  const Tris t65 = lifted(random_tris(65, 1.5f, 0.3f));
  FlatScene A = guarded(scene_of(t65, Tris()));
  const uint32_t begin0 = A.guards[0].tri_begin;
  const size_t tris0 = A.tris.size();
  CHECK(A.guards[0].tri_cap == 65, "at create tri_cap is the count");
  {  // 1. shrink in place
    const Tris t = lifted(random_tris(5, 1.f, 0.3f));
    const Moves mv = replace_on_host(A, 0, t);
    CHECK(!mv.tris && !mv.nodes && A.guards[0].tri_begin == begin0 && A.guards[0].tri_cap == 65 && A.tris.size() == tris0, "65 -> 5 moved something");
    same_scene("65 -> 5", A, guarded(scene_of(t, Tris())), {t});
    line("65 -> 5", A, 0, mv);
  }
  // 2. past tri_cap once, then inside the doubled room, then past it again
  A = guarded(scene_of(t65, Tris()));
  const struct { uint32_t n; bool moves; uint32_t cap; } row[] = {{66, true, 130}, {67, false, 130}, {130, false, 130}, {131, true, 260}};
  for (const auto &r : row) {
    const Tris t = lifted(random_tris(r.n, 1.5f, 0.3f));
    const uint32_t begin_before = A.guards[0].tri_begin;
    const size_t size_before = A.tris.size();
    const Moves mv = replace_on_host(A, 0, t);
    const std::string what = "-> " + std::to_string(r.n);
    CHECK(mv.tris == r.moves && A.guards[0].tri_cap == r.cap, "%s: tris_moved %d, tri_cap %u", what.c_str(), (int)mv.tris, A.guards[0].tri_cap);
    CHECK(A.guards[0].tri_begin == (r.moves ? size_before : begin_before) && A.tris.size() == size_before + (r.moves ? r.cap + CTR_GUARD_SLOTS : 0u), "%s: where the range lies", what.c_str());
    same_scene(what.c_str(), A, guarded(scene_of(t, Tris())), {t});
    line(what.c_str(), A, 0, mv);
  }
  {  // 3. the node range moves without the triangle range: the host's builder with leaves of one triangle
    A = guarded(scene_of(t65, Tris()));
    const uint32_t cap0 = A.guards[0].node_cap, node_begin0 = A.guards[0].node_begin;
    const size_t nodes0 = A.nodes4.size();
    const Moves mv = replace_on_host(A, 0, t65, 1);
    const MeshGuard &g = A.guards[0];
    CHECK(!mv.tris && mv.nodes && g.tri_begin == begin0 && g.node_begin == nodes0 && g.node_begin != node_begin0 && g.node_count > cap0 && g.node_cap == std::max(g.node_count, 2 * cap0) &&
          A.nodes4.size() == nodes0 + g.node_cap + 1u, "leaf size 1: nodes (%u, %u of %u), before %u", g.node_begin, g.node_count, g.node_cap, cap0);
    same_scene("65 -> 65, leaf size 1", A, guarded(scene_of(t65, Tris())), {t65}, false);
    line("65 -> 65, leaf size 1", A, 0, mv);
    // a tree of the usual size afterwards stays in the new range
    const Tris t = lifted(random_tris(70, 1.5f, 0.3f));
    const Moves mv2 = replace_on_host(A, 0, t);
    CHECK(mv2.tris && !mv2.nodes && A.guards[0].node_begin == nodes0, "65 -> 70 after the node move");
    same_scene("65 -> 70 after the node move", A, guarded(scene_of(t, Tris())), {t});
    line("65 -> 70 after the node move", A, 0, mv2);
  }
  {  // 7. one triangle
    const Tris one = lifted(random_tris(1, 1.f, 0.4f)), other = lifted(random_tris(1, 1.f, 0.4f)), many = lifted(random_tris(1000, 2.f, 0.2f));
    A = guarded(scene_of(one, Tris()));
    Moves mv = replace_on_host(A, 0, other);
    CHECK(!mv.tris && !mv.nodes, "1 -> 1 moved something");
    same_scene("1 -> 1", A, guarded(scene_of(other, Tris())), {other});
    line("1 -> 1", A, 0, mv);
    mv = replace_on_host(A, 0, many);
    CHECK(mv.tris && mv.nodes && A.guards[0].tri_cap == 1000, "1 -> 1000");
    same_scene("1 -> 1000", A, guarded(scene_of(many, Tris())), {many});
    line("1 -> 1000", A, 0, mv);
  }
}

// ---- 4: mesh, stand-alone triangle, mesh, sphere; the first mesh grows ----
static void check_mixed() {
  const Tris a = lifted(random_tris(40, 1.f, 0.3f)), b = aside(lifted(random_tris(30, 0.8f, 0.3f), 5.f)), a2 = lifted(random_tris(90, 1.2f, 0.3f));
  const Scene s = scene_of(a, b, true);
  FlatScene A = guarded(s);
  CHECK(A.merged.reserved && !build_merged_tree(A).empty() && A.merged.built, "mixed: the merged tree of two meshes builds");
  guard(A, EYE);
  const FlatScene before = A;
  const Moves mv = replace_on_host(A, 0, a2);
  CHECK(mv.tris && mv.nodes && A.guards[0].tri_begin == before.tris.size() && A.guards[0].node_begin == before.nodes4.size(), "mixed: the first mesh's new ranges are not at the ends");
  // the stand-alone triangle's record is where it was, between the mesh ranges, and what it was
  const DObj &T = A.objs[1], &T0 = before.objs[1];
  CHECK(T.type == CTR_OBJ_TRIANGLE && !memcmp(&T, &T0, sizeof(DObj)) && T.tri_begin > before.guards[0].tri_begin && T.tri_begin < before.guards[1].tri_begin &&
        !memcmp(&A.tris[T.tri_begin], &before.tris[T0.tri_begin], sizeof(DTri)) && !memcmp(&A.gn[4 * (size_t)T.tri_begin], &before.gn[4 * (size_t)T0.tri_begin], 16), "mixed: the stand-alone triangle");
  // the second mesh: its MeshGuard, records, triangles, normals, planes and nodes are untouched
  const MeshGuard &o = A.guards[1], &o0 = before.guards[1];
  CHECK(o.node_begin == o0.node_begin && o.node_count == o0.node_count && o.node_cap == o0.node_cap && o.tri_begin == o0.tri_begin && o.tri_count == o0.tri_count && o.tri_cap == o0.tri_cap &&
        o.obj_index == o0.obj_index && o.mesh_pos == o0.mesh_pos && o.guarded == o0.guarded && o.linear == o0.linear && same_bytes(o.planes, o0.planes), "mixed: the second mesh's MeshGuard");
  CHECK(!memcmp(&A.objs[o.obj_index], &before.objs[o.obj_index], sizeof(DObj)) && !memcmp(&A.meshes[o.mesh_pos], &before.meshes[o.mesh_pos], sizeof(DObj)), "mixed: the second mesh's records");
  CHECK(!memcmp(&A.tris[o.tri_begin], &before.tris[o.tri_begin], (o.tri_count + CTR_GUARD_SLOTS) * sizeof(DTri)) &&
        !memcmp(&A.gn[4 * (size_t)o.tri_begin], &before.gn[4 * (size_t)o.tri_begin], (o.tri_count + CTR_GUARD_SLOTS) * 16), "mixed: the second mesh's triangles");
  CHECK(!memcmp(&A.nodes4[o.node_begin], &before.nodes4[o.node_begin], (o.node_count + 1u) * sizeof(DNode4)), "mixed: the second mesh's nodes");
  // the merged tree's room is where it was
  CHECK(A.merged.tri_begin == before.merged.tri_begin && A.merged.node_begin == before.merged.node_begin && A.merged.tri_count == before.merged.tri_count, "mixed: the merged tree's room moved");
  same_scene("mixed: first mesh 40 -> 90", A, guarded(scene_of(a2, b, true)), {a2, b});
  line("mixed: first mesh 40 -> 90", A, 0, mv);
  // the second mesh afterwards, smaller, then the first again inside its room
  const Tris b2 = aside(lifted(random_tris(7, 0.8f, 0.3f), 5.f)), a3 = lifted(random_tris(150, 1.2f, 0.3f)), a4 = lifted(random_tris(170, 1.2f, 0.3f));
  const Moves mv2 = replace_on_host(A, 1, b2);
  CHECK(!mv2.tris && !mv2.nodes, "mixed: the second mesh 30 -> 7 moved");
  same_scene("mixed: second mesh 30 -> 7", A, guarded(scene_of(a2, b2, true)), {a2, b2});
  line("mixed: second mesh 30 -> 7", A, 1, mv2);
  const Moves mv3 = replace_on_host(A, 0, a3);
  CHECK(mv3.tris && A.guards[0].tri_cap == 180, "mixed: 90 -> 150 moves into a room of 180");
  same_scene("mixed: first mesh 90 -> 150", A, guarded(scene_of(a3, b2, true)), {a3, b2});
  line("mixed: first mesh 90 -> 150", A, 0, mv3);
  const Moves mv4 = replace_on_host(A, 0, a4);
  CHECK(!mv4.tris && A.guards[0].tri_cap == 180, "mixed: 150 -> 170 inside a room of 180");
  same_scene("mixed: first mesh 150 -> 170", A, guarded(scene_of(a4, b2, true)), {a4, b2});
  line("mixed: first mesh 150 -> 170", A, 0, mv4);
}

// ---- 5: triangles in the eye's plane at three counts; 6: the mirror threshold; 8: rebuilds and updates afterwards ----
static void check_guard_states() {
  const Tris a = lifted(random_tris(100, 1.5f, 0.3f)), b = aside(lifted(random_tris(12, 0.5f, 0.4f), 6.f));
  FlatScene A = guarded(scene_of(a, b));
  struct Step { const char *what; Tris tris; size_t guarded; bool linear; uint32_t leaf; } steps[] = {
      {"3 in the eye's plane, of 40", with_in_plane(lifted(random_tris(40, 1.5f, 0.3f)), 3), 3, false, BVH_LEAF},
      {"70 in the eye's plane, of 200", with_in_plane(lifted(random_tris(200, 1.5f, 0.3f)), 70), 0, true, BVH_LEAF},
      {"70 again, of 150, leaf size 2", with_in_plane(lifted(random_tris(150, 1.5f, 0.3f)), 70), 0, true, 2},
      {"none in the plane, of 90", lifted(random_tris(90, 1.5f, 0.3f)), 0, false, BVH_LEAF}};
  Tris now_a = a;
  for (const Step &st : steps) {
    Moves mv{false, false};
    {  // (the payload of a mesh that goes or stays linear covers the NEW tree)
      const MeshTree tree = host_mesh_tree(st.tris.data(), st.tris.size(), st.leaf);
      mesh_replaced(A, 0, (uint32_t)st.tris.size(), tree, &mv.tris, &mv.nodes);
      update_on_host(A, 0, st.tris);
      bool payload = false;
      for (const DirtyRange &r : guard(A, EYE))
        if (r.array == DirtyRange::NODES4 && r.begin == A.guards[0].node_begin && !r.payload.empty()) {
          payload = true;
          CHECK(r.count == A.guards[0].node_count && r.payload.size() == r.count, "%s: payload of %zu nodes for a tree of %u", st.what, r.payload.size(), A.guards[0].node_count);
        }
      CHECK(payload == st.linear, "%s: unbounded payload %s", st.what, payload ? "sent" : "not sent");
      CHECK(guard(A, EYE).empty(), "%s: the same cameras again change nothing", st.what);
    }
    CHECK(A.guards[0].guarded.size() == st.guarded && A.guards[0].linear == st.linear, "%s: guarded %zu linear %d", st.what, A.guards[0].guarded.size(), (int)A.guards[0].linear);
    same_scene(st.what, A, guarded(scene_of(st.tris, b)), {st.tris, b}, st.leaf == BVH_LEAF);
    line(st.what, A, 0, mv);
    now_a = st.tris;
  }
  // 6. the reflecting mesh across CTR_MIRROR_MESH_TRIS both ways: its triangles are mirrors at 12, not at 20, and again at 12
  static_assert(CTR_MIRROR_MESH_TRIS >= 12 && CTR_MIRROR_MESH_TRIS < 20, "the counts of case 6 straddle the threshold");
  Tris now_b = b;
  for (uint32_t n : {20u, 12u}) {
    now_b = aside(lifted(random_tris(n, 0.5f, 0.4f), 6.f));
    const Moves mv = replace_on_host(A, 1, now_b);
    const FlatScene B = guarded(scene_of(now_a, now_b));
    const size_t origins = plan_guards(A, cams_of(scene_of(now_a, now_b).desc)).n_origins;
    CHECK(origins == plan_guards(B, cams_of(scene_of(now_a, now_b).desc)).n_origins && (n > CTR_MIRROR_MESH_TRIS) == (origins == 1), "mirror mesh of %u: %zu ray origins", n, origins);
    const std::string what = "reflecting mesh -> " + std::to_string(n);
    same_scene(what.c_str(), A, B, {now_a, now_b});
    line(what.c_str(), A, 1, mv);
    printf("mirror mesh of %u: origins %zu\n", n, origins);
  }
  // 8. after the replaces a rebuild and an update at the NEW count hold what they held before
  {
    const Tris am = moved(now_a, 0.8f, 0.1f);
    bool was_moved = false;
    mesh_rebuilt(A, 0, host_mesh_tree(am.data(), am.size()), &was_moved);
    update_on_host(A, 0, am);
    guard(A, EYE);
    CHECK(!was_moved, "a rebuild at the new count moved the tree");
    same_scene("rebuild after replaces", A, guarded(scene_of(am, now_b)), {am, now_b}, true, false);
    // (mesh_rebuilt counts every record of the arrays, as it always has; the live records are what same_scene compares)
    printf("rebuild after replaces: moved %d\n", (int)was_moved);
    const Tris au = moved(am, -0.2f, 0.0f);
    update_on_host(A, 0, au);
    guard(A, EYE);
    // an update keeps the tree's shape: the fresh scene's tree is another one, the mesh is the same
    same_scene("update after replaces", A, guarded(scene_of(au, now_b)), {au, now_b}, false, false);
    printf("update after replaces: holds\n");
  }
}

int main() {
  check_counts();
  check_mixed();
  check_guard_states();
  printf(fails ? "mesh_replace_check: %d FAILURES\n" : "mesh_replace_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
