// mesh_update_check.cpp — the host-checkable half of ctr_scene_update_mesh (include/cutrace_update.h) without a device; meant to run
// under ASan/UBSan as well.  tests/test_mesh_update_cpu.py builds and runs it and reads the lines it prints.
//
//   schedule   level_schedule (cutrace_amd/csrc/mesh_refit.h) on trees from bvh4_build over random and degenerate triangle sets:
//              every node in exactly one level, every inner child in a strictly lower level than its parent, at most
//              BVH4_MAX_DEPTH + 1 levels, a one-node mesh gives one level
//   refit      refit_slot over the schedule with MOVED vertices: every used slot's box equals the brute-force min / max over
//              the vertices of all triangles below it (as values: -0 = +0), the root's union equals ctr_mesh_bounds
//   identity   the refit with UNMOVED vertices against the builder's own boxes, as values and as bytes (the line says which)
//   records    tri_record.h compiled for the host against flatten_scene's tris, gn and planes of a mesh, byte for byte
//   update     the whole update restated on the host (update_tris and refit_level through the shared headers, then
//              mesh_updated and the guard) against a scene flattened from the replaced triangles: per FILE triangle the same
//              record, normal and plane bytes, the same boxes, the same guarded triangles, and a mesh that is linear before
//              and after an update gets its unbounded payload again
#include <set>

#include "edit_check_common.h"

static std::vector<BvhInput> boxes_of(const Tris &t) {
  std::vector<BvhInput> prims(t.size());
  for (size_t q = 0; q < t.size(); q++) {
    const float *v = &t[q].p1.x;
    for (int a = 0; a < 3; a++) {
      prims[q].mn[a] = fminf(v[a], fminf(v[3 + a], v[6 + a]));
      prims[q].mx[a] = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
      prims[q].c[a] = 0.5f * (prims[q].mn[a] + prims[q].mx[a]);
    }
  }
  return prims;
}

static void check_tree(const char *what, const Tris &tris, bool zero_free) {
  std::vector<DNode4> nodes;
  std::vector<uint32_t> order;
  bvh4_build(boxes_of(tris), BVH_LEAF, nodes, order);
  const uint32_t n = (uint32_t)tris.size(), nn = (uint32_t)nodes.size();
  // ---- schedule ----
  LevelSchedule S;
  CHECK(level_schedule(nodes.data(), nn, n, S), "%s: no schedule", what);
  if (S.levels() == 0) return;
  std::vector<int> level(nn, -1);
  for (size_t h = 0; h < S.levels(); h++)
    for (uint32_t i = S.begin[h]; i < S.begin[h + 1]; i++) {
      CHECK(S.nodes[i] < nn && level[S.nodes[i]] == -1, "%s: node %u twice or out of range", what, S.nodes[i]);
      if (S.nodes[i] < nn) level[S.nodes[i]] = (int)h;
    }
  CHECK(S.begin.back() == nn && S.nodes.size() == nn, "%s: %u of %u nodes scheduled", what, S.begin.back(), nn);
  for (uint32_t i = 0; i < nn; i++) {
    CHECK(level[i] >= 0, "%s: node %u in no level", what, i);
    bool all_leaves = true;
    for (int c = 0; c < 4; c++)
      if (!(nodes[i].child[c] & BVH_LEAF_FLAG)) {
        all_leaves = false;
        CHECK(level[nodes[i].child[c]] < level[i], "%s: child %u of node %u is not in a lower level", what, nodes[i].child[c], i);
      }
    CHECK(all_leaves == (level[i] == 0), "%s: node %u: level 0 means every used child is a leaf", what, i);
  }
  CHECK(S.levels() <= BVH4_MAX_DEPTH + 1, "%s: %zu levels", what, S.levels());
  if (nn == 1) CHECK(S.levels() == 1, "%s: a one-node mesh has %zu levels", what, S.levels());
  // ---- the records the refit reads `orig` from ----
  std::vector<DTri> recs(n);
  float gn[4];
  for (uint32_t k = 0; k < n; k++) make_tri(tris[order[k]].p1, tris[order[k]].p2, tris[order[k]].p3, order[k], recs[k], gn);
  // ---- identity refit against the builder's boxes ----
  std::vector<DNode4> same(nodes);
  refit_on_host(same.data(), S, recs.data(), tris);
  size_t value_diff = 0, byte_diff = 0;
  for (uint32_t i = 0; i < nn; i++)
    for (int c = 0; c < 4; c++)
      for (int a = 0; a < 3; a++) {
        value_diff += !(same[i].lo[a][c] == nodes[i].lo[a][c]) + !(same[i].hi[a][c] == nodes[i].hi[a][c]);
        byte_diff += (memcmp(&same[i].lo[a][c], &nodes[i].lo[a][c], 4) != 0) + (memcmp(&same[i].hi[a][c], &nodes[i].hi[a][c], 4) != 0);
      }
  CHECK(value_diff == 0, "%s: identity refit changes %zu box values", what, value_diff);
  if (zero_free) CHECK(byte_diff == 0, "%s: identity refit changes %zu box words of a mesh without a zero coordinate", what, byte_diff);
  for (uint32_t i = 0; i < nn; i++)  // (everything but the boxes is untouched)
    CHECK(!memcmp(same[i].child, nodes[i].child, sizeof(nodes[i].child)) && same[i].axis == nodes[i].axis, "%s: node %u: children or axis changed", what, i);
  // ---- refit with moved vertices against brute force ----
  const Tris mv = moved(tris, 0.7f, 0.05f);
  std::vector<DNode4> re(nodes);
  refit_on_host(re.data(), S, recs.data(), mv);
  for (uint32_t i = 0; i < nn; i++)
    for (int c = 0; c < 4; c++) {
      if (re[i].child[c] == BVH_LEAF_FLAG) {
        for (int a = 0; a < 3; a++) CHECK(re[i].lo[a][c] == nodes[i].lo[a][c] && re[i].hi[a][c] == nodes[i].hi[a][c], "%s: empty slot touched", what);
        continue;
      }
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      brute(re, re[i].child[c], order, mv, lo, hi);
      for (int a = 0; a < 3; a++) CHECK(re[i].lo[a][c] == lo[a] && re[i].hi[a][c] == hi[a], "%s: node %u slot %d axis %d: box is not the min / max of what lies below", what, i, c, a);
    }
  float box[6];
  refit_mesh_box(re[0], box);
  ctr_vec3 mn, mx;
  ctr_mesh_bounds(mv.data(), mv.size(), &mn, &mx);
  CHECK(box[0] == mn.x && box[1] == mn.y && box[2] == mn.z && box[3] == mx.x && box[4] == mx.y && box[5] == mx.z, "%s: the root's union is not ctr_mesh_bounds", what);
  printf("tree %-28s triangles %6u nodes %6u levels %2zu identity_value_diff %zu identity_byte_diff %zu\n", what, n, nn, S.levels(), value_diff, byte_diff);
}

// ---- a small scene: a mesh of `a`, a plane, a reflective mesh of `b`, one light ----
static Scene scene_of(const Tris &a, const Tris &b) {
  Scene s;
  ctr_material m{};
  m.type = CTR_MAT_PHONG;
  m.color = ctr_vec3{0.5f, 0.5f, 0.5f};
  s.materials.push_back(m);
  m.reflexivity = 0.5f;
  s.materials.push_back(m);
  ctr_light l{};
  l.type = CTR_LIGHT_POINT;
  l.v = ctr_vec3{5.f, 6.f, 7.03f};
  s.lights.push_back(l);
  s.mesh(a, 0);
  s.plane(ctr_vec3{0, -9, 0}, ctr_vec3{0, 1, 0}, 0);
  s.mesh(b, 1);
  s.cam.w = s.cam.h = 16;
  s.finish();
  return s;
}

// the mesh's records, normals and planes of A and B agree per FILE triangle; its boxes and the scene's agree as values
static void same_mesh(const char *what, const FlatScene &A, const FlatScene &B, size_t gi) {
  const MeshGuard &ga = A.guards[gi], &gb = B.guards[gi];
  CHECK(ga.tri_count == gb.tri_count, "%s: counts", what);
  std::vector<uint32_t> at_b(gb.tri_count);
  for (uint32_t k = 0; k < gb.tri_count; k++) at_b[B.tris[gb.tri_begin + k].orig] = k;
  size_t bad = 0;
  for (uint32_t k = 0; k < ga.tri_count; k++) {
    const uint32_t f = A.tris[ga.tri_begin + k].orig, kb = at_b[f];
    bad += memcmp(&A.tris[ga.tri_begin + k], &B.tris[gb.tri_begin + kb], sizeof(DTri)) != 0;
    bad += memcmp(&A.gn[4 * (ga.tri_begin + f)], &B.gn[4 * (gb.tri_begin + f)], 16) != 0;
    bad += memcmp(&ga.planes[CTR_PLANE_DOUBLES * k], &gb.planes[CTR_PLANE_DOUBLES * kb], CTR_PLANE_DOUBLES * sizeof(double)) != 0;
  }
  CHECK(bad == 0, "%s: %zu records, normals or planes differ from the fresh scene's", what, bad);
  for (int q = 0; q < 6; q++) {
    CHECK(A.objs[ga.obj_index].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in objs", what, q);
    CHECK(A.meshes[ga.mesh_pos].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in meshes", what, q);
  }
  for (size_t k = A.n_mesh + 1; k < A.meshes.size(); k++)
    if (A.meshes[k].index == ga.obj_index)
      for (int q = 0; q < 6; q++) CHECK(A.meshes[k].f[q] == B.objs[gb.obj_index].f[q], "%s: box word %d in the scene-order copy", what, q);
  for (int a = 0; a < 3; a++) CHECK(A.tl_mn[a] == B.tl_mn[a] && A.tl_mx[a] == B.tl_mx[a], "%s: tl_mn / tl_mx", what);
  // the guard picks the same FILE triangles
  std::set<uint32_t> fa, fb;
  for (uint32_t t : ga.guarded) fa.insert(A.tris[ga.tri_begin + t].orig);
  for (uint32_t t : gb.guarded) fb.insert(B.tris[gb.tri_begin + t].orig);
  CHECK(fa == fb && ga.linear == gb.linear, "%s: guarded %zu / %zu triangles, linear %d / %d", what, fa.size(), fb.size(), (int)ga.linear, (int)gb.linear);
  CHECK(A.objs[ga.obj_index].bvh_root == (ga.guarded.empty() ? 0u : ga.node_count), "%s: bvh_root", what);
  printf("update %-36s guarded %2zu linear %d\n", what, fa.size(), (int)ga.linear);
}

// every top-level box is the union of the mesh boxes below it
static void top_level_holds(const char *what, const FlatScene &F, uint32_t d, float *lo, float *hi) {
  if (d & BVH_LEAF_FLAG) {
    for (uint32_t k = d & 0xFFFFFFu; k < (d & 0xFFFFFFu) + ((d >> 24) & 0x7Fu); k++)
      for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], F.meshes[k].f[a]); hi[a] = std::max(hi[a], F.meshes[k].f[3 + a]); }
    return;
  }
  const DNode &N = F.nodes[F.tlas_begin + d];
  const uint32_t kid[2] = {N.left, N.right};
  for (int c = 0; c < 2; c++) {
    float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    top_level_holds(what, F, kid[c], l, h);
    for (int a = 0; a < 3; a++) {
      CHECK(N.mn[a][c] == l[a] && N.mx[a][c] == h[a], "%s: top-level node %u child %d axis %d", what, d, c, a);
      lo[a] = std::min(lo[a], l[a]); hi[a] = std::max(hi[a], h[a]);
    }
  }
}

static void check_records_and_update() {
  const float eye[3] = {0.3f, 0.2f, 0.5f};
  Tris a = random_tris(150, 1.5f, 0.3f), b = random_tris(12, 0.5f, 0.4f);
  for (ctr_triangle &t : a) { t.p1.z += 3.f; t.p2.z += 3.f; t.p3.z += 3.f; }  // (off the plane z = 0.5)
  a.push_back(ctr_triangle{{0.1f, 0.1f, 2.f}, {0.1f, 0.1f, 2.f}, {0.1f, 0.1f, 2.f}});  // zero area: a point, three points of a line
  a.push_back(ctr_triangle{{0, 0, 2.f}, {0.5f, 0.5f, 2.f}, {1, 1, 2.f}});
  const Scene s0 = scene_of(a, b);
  FlatScene A = flat_of(s0.desc);
  // ---- records: tri_record.h against flatten_scene, byte for byte ----
  size_t bad = 0;
  for (const MeshGuard &g : A.guards) {
    const ctr_triangle *src = s0.triangles.data() + s0.objects[g.obj_index].tri_begin;
    for (uint32_t k = 0; k < g.tri_count; k++) {
      const uint32_t f = A.tris[g.tri_begin + k].orig;
      DTri T;
      float gn[4];
      double q[CTR_PLANE_DOUBLES];
      make_tri(src[f].p1, src[f].p2, src[f].p3, f, T, gn);
      guard_plane(src[f].p1, src[f].p2, src[f].p3, q);
      bad += memcmp(&T, &A.tris[g.tri_begin + k], sizeof(T)) != 0;
      bad += memcmp(gn, &A.gn[4 * (g.tri_begin + f)], sizeof(gn)) != 0;
      bad += memcmp(q, &g.planes[CTR_PLANE_DOUBLES * k], sizeof(q)) != 0;
    }
  }
  CHECK(bad == 0, "records: %zu differ from flatten_scene's", bad);
  printf("records tri_record.h against flatten_scene: %zu differ\n", bad);
  // ---- updates in a row: moved, 3 in the eye's plane, 70 (linear), 70 again (linear stays: payload again), none ----
  guard(A, eye);
  CHECK(!build_merged_tree(A).empty() && A.merged.built, "the merged tree of two meshes builds");
  guard(A, eye);
  struct Step { const char *what; Tris tris; bool linear; } steps[] = {
      {"moved", moved(a, 0.5f, 0.02f), false}, {"3 in the eye's plane", with_in_plane(a, 3), false}, {"70 in the eye's plane", with_in_plane(a, 70), true},
      {"70 again: linear payload after refit", with_in_plane(moved(a, 0.1f, 0.0f), 70), true}, {"none in the plane", moved(a, -0.3f, 0.01f), false}};
  for (const Step &st : steps) {
    for (const ctr_triangle &t : st.tris)
      for (int j = 0; j < 9; j++) CHECK(std::isfinite((&t.p1.x)[j]), "test input");
    update_on_host(A, 0, st.tris);
    CHECK(!A.merged.reserved && !A.merged.built && !A.merged.usable && A.merged.src.empty(), "%s: the merged tree is retired", st.what);
    CHECK(build_merged_tree(A).empty(), "%s: a retired merged tree is never built", st.what);
    const std::vector<DirtyRange> dirty = guard(A, eye);
    bool payload = false;
    for (const DirtyRange &r : dirty)
      if (r.array == DirtyRange::NODES4 && r.begin == A.guards[0].node_begin && !r.payload.empty()) {
        payload = true;
        for (const DNode4 &N : r.payload)
          for (int c = 0; c < 4; c++)
            if (N.child[c] != BVH_LEAF_FLAG) CHECK(N.lo[0][c] == -3.0e38f && N.hi[2][c] == 3.0e38f, "%s: payload slot not unbounded", st.what);
      }
    CHECK(payload == st.linear, "%s: unbounded payload %s", st.what, payload ? "sent" : "not sent");
    CHECK(guard(A, eye).empty(), "%s: the same cameras again change nothing", st.what);
    const Scene s1 = scene_of(st.tris, b);
    FlatScene B = flat_of(s1.desc);
    guard(B, eye);
    same_mesh(st.what, A, B, 0);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    top_level_holds(st.what, A, A.tlas_root, lo, hi);
    for (int q = 0; q < 3; q++) CHECK(lo[q] == A.tl_mn[q] && hi[q] == A.tl_mx[q], "%s: tl box", st.what);
    // the host copy keeps REAL boxes also while the device has the unbounded payload
    const MeshGuard &g = A.guards[0];
    for (uint32_t i = 0; i < g.node_count; i++)
      for (int c = 0; c < 4; c++)
        if (A.nodes4[g.node_begin + i].child[c] != BVH_LEAF_FLAG) CHECK(A.nodes4[g.node_begin + i].hi[0][c] < 1e30f, "%s: host copy lost a real box", st.what);
  }
  // ---- the reflective 12-triangle mesh moves: its triangles are mirrors, the virtual eyes follow ----
  const Tris b2 = moved(b, 1.0f, 0.0f);
  update_on_host(A, 1, b2);
  guard(A, eye);
  const Scene s2 = scene_of(steps[4].tris, b2);
  FlatScene B = flat_of(s2.desc);
  guard(B, eye);
  same_mesh("reflective mesh moved", A, B, 1);
  same_mesh("reflective mesh moved: the other mesh", A, B, 0);
  const GuardPlan pa = plan_guards(A, std::vector<DCam>(1, DCam{})), pb = plan_guards(B, std::vector<DCam>(1, DCam{}));
  CHECK(pa.n_mirrors == pb.n_mirrors && pa.n_origins == pb.n_origins && pa.n_mirrors > 0, "mirrors %zu / %zu, origins %zu / %zu", pa.n_mirrors, pb.n_mirrors, pa.n_origins, pb.n_origins);
}

int main() {
  rng.seed(11);  // (this program's own seed: before the first draw)
  auto flat_set = [](size_t n) { Tris t = random_tris(n, 5.f, 0.4f); for (ctr_triangle &q : t) q.p1.x = q.p2.x = q.p3.x = 1.25f; return t; };
  auto cluster = [](size_t n) {  // triangle sizes over many octaves: the SAH tree is too deep, bvh4_build falls back to the depth-bounded rebuild
    Tris t = random_tris(n, 1.f, 0.01f);
    for (size_t i = 0; i < t.size(); i++) {
      const float s = std::ldexp(1.0f, -(int)(i % 120));
      for (int j = 0; j < 9; j++) (&t[i].p1.x)[j] *= s;
    }
    return t;
  };
  for (size_t n : {1u, 4u, 5u, 64u, 65u, 1000u, 20000u}) check_tree(("random " + std::to_string(n)).c_str(), random_tris(n, 10.f, 0.5f), true);
  check_tree("coincident points", Tris(300, ctr_triangle{{1, 2, 3}, {1, 2, 3}, {1, 2, 3}}), true);
  check_tree("flat in x", flat_set(2000), true);
  check_tree("with zero coordinates", [] { Tris t = random_tris(500, 2.f, 0.5f); for (size_t i = 0; i < t.size(); i += 3) { t[i].p1.y = 0.f; t[i].p2.z = -0.f; } return t; }(), false);
  check_tree("geometric cluster", cluster(5000), true);
  check_records_and_update();
  printf(fails ? "mesh_update_check: %d FAILURES\n" : "mesh_update_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
