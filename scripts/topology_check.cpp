// topology_check.cpp — the host-checkable half of include/cutrace_topology.h (ctr_scene_add_object, ctr_scene_add_mesh,
// ctr_scene_remove_object) without a device; meant to run under ASan/UBSan as well.  tests/test_topology_cpu.py builds and runs it and
// reads the lines it prints.
//
// A flattened scene goes through adds and removes on the host copy — object_added, mesh_added with the update's steps behind it
// (update_on_host) and mesh_joined, object_removed (scene_flatten.cpp), then the guard — and after each step it is compared with
// flatten_scene of the edited description: the removed objects deleted, the added ones appended.  Byte for byte what holds no range:
// oloop (but for a stand-alone triangle's record index), planes, n_axis_recs, the top-level nodes, tlas_root, tl_mn / tl_mx, lights,
// materials, the shading flags, n_mesh, has_mesh, mesh_tris, ray_slots, live_mesh_bytes.  Relative to their ranges, as
// mesh_replace_check.cpp compares a replaced scene: objs and meshes apart from where the ranges begin, and per mesh its records,
// normals, planes, guard records, nodes and box.  Every tree is the host builder's own at its default leaf size, so the nodes agree
// byte for byte.  Also: the ranges are disjoint and inside their arrays, and the free list holds exactly what no object owns.
#include <set>

#include "edit_check_common.h"

static const float EYE[3] = {0.3f, 0.2f, -0.5f};  // room_scene's eye (tests/live.py): its image in a reflecting wall z = 0 lies in z = 0.5

// ---- the description that is edited alongside the host copy ----
struct Item { ctr_object o; Tris tris; };
struct Model {
  std::vector<Item> items;
  std::vector<ctr_light> lights;
  std::vector<ctr_material> materials;
};
enum { OPAQUE = 0, OTHER = 1, GLASS = 2, MIRROR = 3 };

static Item sphere(ctr_vec3 c, float r, uint64_t mat) { Scene s; s.sphere(c, r, mat); return {s.objects[0], {}}; }
static Item plane(ctr_vec3 p, ctr_vec3 n, uint64_t mat) { Scene s; s.plane(p, n, mat); return {s.objects[0], {}}; }
static Item triangle(ctr_vec3 a, ctr_vec3 b, ctr_vec3 c, uint64_t mat) { Scene s; s.triangle(a, b, c, mat); return {s.objects[0], {}}; }
static Item mesh(const Tris &t, uint64_t mat) { Scene s; s.mesh(t, mat); return {s.objects[0], t}; }

static Scene describe(const Model &m) {
  Scene s;
  s.lights = m.lights;
  s.materials = m.materials;
  for (const Item &it : m.items) {
    if (it.o.type == CTR_OBJ_MESH) s.mesh(it.tris, it.o.mat_idx);
    else s.objects.push_back(it.o);
  }
  s.cam.pos = ctr_vec3{EYE[0], EYE[1], EYE[2]};
  s.cam.w = s.cam.h = 16;
  s.finish();
  return s;
}

static Tris shifted(Tris t, float dx, float dy = 0.f, float dz = 0.f) {
  for (ctr_triangle &q : t)
    for (ctr_vec3 *v : {&q.p1, &q.p2, &q.p3}) { v->x += dx; v->y += dy; v->z += dz; }
  return t;
}

static Model empty_model() {
  Model m;
  m.lights = {light(CTR_LIGHT_POINT, 3.f, -1.f, 1.f, 0.9f), light(CTR_LIGHT_SUN, 0.3f, -0.8f, 0.5f, 0.3f)};
  m.materials = {material(0.f, 0.f, 40.f), material(0.f, 0.f, 10.f), material(0.f, 0.5f, 20.f), material(0.4f, 0.f, 30.f)};
  return m;
}

static const ctr_vec3 WALLS[5][2] = {{{-5, 0, 0}, {1, 0, 0}}, {{5, 0, 0}, {-1, 0, 0}}, {{0, -3, 0}, {0, 1, 0}}, {{0, 8, 0}, {0, -1, 0}}, {{0, 0, -6}, {0, 0, 1}}};

// room_scene of tests/live.py: planes at 0, 1, 3, 5, 8; the 70-triangle mesh with five triangles in z = 0.5 at 2; a sphere at 4; the
// reflecting 12-triangle mesh at 6; a stand-alone triangle at 7
enum { ROOM_MESH = 2, ROOM_SPHERE = 4, ROOM_SMALL = 6, ROOM_TRI = 7, ROOM_WALL = 8 };
static Model room_model() {
  Model m = empty_model();
  m.items = {plane(WALLS[0][0], WALLS[0][1], OTHER), plane(WALLS[1][0], WALLS[1][1], OTHER), mesh(guard_tris(5, 65, false), OPAQUE),
             plane(WALLS[2][0], WALLS[2][1], OTHER), sphere(ctr_vec3{-2.f, -1.f, 3.f}, 0.7f, OPAQUE), plane(WALLS[3][0], WALLS[3][1], OTHER),
             mesh(shifted(guard_tris(0, 12, false), 2.5f), MIRROR), triangle(ctr_vec3{-3, 0, 6}, ctr_vec3{-2, 0.5f, 6.5f}, ctr_vec3{-2.5f, 2, 6}, OPAQUE),
             plane(WALLS[4][0], WALLS[4][1], OTHER)};
  return m;
}

static FlatScene guarded(const Model &m) {
  const Scene s = describe(m);
  FlatScene F = flat_of(s.desc);
  guard(F, EYE);
  return F;
}

// ---- the three calls on the host copy ----
struct Added { bool tris_reused = false, nodes_reused = false; uint32_t tri_cap = 0; };

static Added add(FlatScene &A, Model &m, const Item &it) {
  Added ad;
  std::string err;
  if (it.o.type != CTR_OBJ_MESH) {
    CHECK(check_new_object(A, it.o, err) == CTR_OK, "a good object is refused: %s", err.c_str());
    const size_t before = A.tris.size();
    object_added(A, it.o, &ad.tris_reused);
    CHECK(A.tris.size() == before + (it.o.type == CTR_OBJ_TRIANGLE && !ad.tris_reused ? 1u : 0u), "an added object grew tris by something else than its record");
  } else {
    const MeshTree tree = host_mesh_tree(it.tris.data(), it.tris.size());
    const AddRoom room = add_room(A, (uint32_t)it.tris.size(), (uint32_t)tree.nodes.size());
    mesh_added(A, it.o.mat_idx, (uint32_t)it.tris.size(), tree);
    const size_t gi = A.guards.size() - 1;
    const MeshGuard &g = A.guards[gi];
    CHECK(A.tris.size() == room.tris_after && A.gn.size() == 4 * room.tris_after && A.nodes4.size() == room.nodes4_after && g.tri_begin == room.tri_begin &&
          g.tri_cap == room.tri_cap && g.node_begin == room.node_begin && g.node_cap == room.node_cap && g.mesh_pos < 0, "add_room does not say what mesh_added did");
    update_on_host(A, gi, it.tris);  // (its mesh_updated finds a mesh that nothing walks yet, and leaves it)
    float box[6];
    refit_mesh_box(A.nodes4[A.guards[gi].node_begin], box);
    mesh_joined(A, gi, box);
    ad.tris_reused = room.tris_reused;
    ad.nodes_reused = room.nodes_reused;
    ad.tri_cap = room.tri_cap;
  }
  m.items.push_back(it);
  guard(A, EYE);
  return ad;
}

static void remove(FlatScene &A, Model &m, size_t i) {
  long gi = -2;
  const size_t guards_before = A.guards.size();
  object_removed(A, i, &gi);
  CHECK((gi >= 0) == (m.items[i].o.type == CTR_OBJ_MESH) && A.guards.size() == guards_before - (gi >= 0 ? 1u : 0u), "remove %zu: guard_removed %ld", i, gi);
  m.items.erase(m.items.begin() + i);
  guard(A, EYE);
}

// ---- the comparison ----
typedef std::vector<std::pair<size_t, size_t>> Ranges;

// owned, freed and the merged tree's room: disjoint, inside the arrays, and together every record of them
static void ranges_hold(const char *what, const FlatScene &A) {
  Ranges tr, nd;
  for (const DObj &O : A.objs)
    if (O.type == CTR_OBJ_TRIANGLE) tr.push_back({O.tri_begin, O.tri_begin + 1u});
  for (const MeshGuard &g : A.guards) {
    if (g.tri_cap) tr.push_back({g.tri_begin, (size_t)g.tri_begin + g.tri_cap + CTR_GUARD_SLOTS});
    nd.push_back({g.node_begin, (size_t)g.node_begin + g.node_cap + 1u});
    CHECK(g.tri_count <= g.tri_cap && g.node_count <= g.node_cap, "%s: a count above its room", what);
  }
  const SceneRoom room = scene_room(A);
  size_t live_t = 0, live_n = 0;
  for (const auto &r : tr) live_t += r.second - r.first;
  for (const auto &r : nd) live_n += r.second - r.first;
  CHECK(room.tris_live == live_t && room.nodes4_live == live_n && room.tris_total == A.tris.size() && room.nodes4_total == A.nodes4.size(),
        "%s: scene_room says %llu of %llu and %llu of %llu", what, (unsigned long long)room.tris_live, (unsigned long long)room.tris_total,
        (unsigned long long)room.nodes4_live, (unsigned long long)room.nodes4_total);
  for (size_t k = 0; k < A.free_tris.size(); k++) {
    tr.push_back({A.free_tris[k].begin, (size_t)A.free_tris[k].begin + A.free_tris[k].count});
    if (k) CHECK(A.free_tris[k - 1].begin < A.free_tris[k].begin, "%s: free_tris is not in address order", what);
  }
  for (size_t k = 0; k < A.free_nodes4.size(); k++) {
    nd.push_back({A.free_nodes4[k].begin, (size_t)A.free_nodes4[k].begin + A.free_nodes4[k].count});
    if (k) CHECK(A.free_nodes4[k - 1].begin < A.free_nodes4[k].begin, "%s: free_nodes4 is not in address order", what);
  }
  if (A.merged.tri_count) {  // the merged tree's room, reserved at create and retired since
    tr.push_back({A.merged.tri_begin, (size_t)A.merged.tri_begin + A.merged.tri_count + CTR_GUARD_SLOTS});
    nd.push_back({A.merged.node_begin, (size_t)A.merged.node_begin + A.merged.node_cap + CTR_MERGED_SPARE_NODES});
  }
  auto tile = [&](Ranges &r, size_t size, const char *name) {
    std::sort(r.begin(), r.end());
    size_t at = 0;
    for (const auto &q : r) {
      CHECK(q.first == at, "%s: %s records %zu .. %zu are %s", what, name, std::min(at, q.first), std::max(at, q.first), q.first > at ? "neither owned nor free" : "in two ranges");
      at = q.second;
    }
    CHECK(at == size, "%s: the %s ranges end at %zu in an array of %zu", what, name, at, size);
  };
  tile(tr, A.tris.size(), "triangle");
  tile(nd, A.nodes4.size(), "node");
  CHECK(A.gn.size() == 4 * A.tris.size(), "%s: gn has %zu floats for %zu records", what, A.gn.size(), A.tris.size());
}

// mesh gi of A (edited) against mesh gi of B (fresh), relative to their ranges
static void same_mesh(const char *what, const FlatScene &A, const FlatScene &B, size_t gi, const Tris &nt) {
  const MeshGuard &ga = A.guards[gi], &gb = B.guards[gi];
  CHECK(ga.tri_count == gb.tri_count && ga.tri_count == nt.size() && ga.obj_index == gb.obj_index && ga.mesh_pos == gb.mesh_pos && ga.node_count == gb.node_count,
        "%s: mesh %zu: count %u / %u, object %u / %u, leaf %d / %d", what, gi, ga.tri_count, gb.tri_count, ga.obj_index, gb.obj_index, ga.mesh_pos, gb.mesh_pos);
  if (ga.tri_count != gb.tri_count || ga.node_count != gb.node_count || ga.mesh_pos != gb.mesh_pos) return;
  CHECK(same_bytes(ga.planes, gb.planes), "%s: mesh %zu: guard planes", what, gi);
  const size_t n = ga.tri_count;
  // records (leaf order), the guard records behind them, normals (file order inside the range)
  // (a spare record beyond the current guard state, and the spare node of a mesh with none, are whatever the last state left)
  const size_t recs = n + ga.guarded.size();
  CHECK(!recs || (!memcmp(&A.tris[ga.tri_begin], &B.tris[gb.tri_begin], recs * sizeof(DTri)) && !memcmp(&A.gn[4 * (size_t)ga.tri_begin], &B.gn[4 * (size_t)gb.tri_begin], recs * 16)),
        "%s: mesh %zu: records, spare records or normals differ from the fresh scene's", what, gi);
  CHECK(ga.guarded == gb.guarded && ga.linear == gb.linear, "%s: mesh %zu: guarded %zu / %zu, linear %d / %d", what, gi, ga.guarded.size(), gb.guarded.size(), (int)ga.linear, (int)gb.linear);
  // nodes and the spare node; what remains of a reused range is empty
  CHECK(!memcmp(&A.nodes4[ga.node_begin], &B.nodes4[gb.node_begin], ((size_t)ga.node_count + (ga.guarded.empty() ? 0u : 1u)) * sizeof(DNode4)), "%s: mesh %zu: nodes or the spare node", what, gi);
  const DNode4 empty = empty_node4();
  for (uint32_t k = ga.node_count + 1u; k <= ga.node_cap; k++) CHECK(!memcmp(&A.nodes4[ga.node_begin + k], &empty, sizeof(empty)), "%s: mesh %zu: unused node %u of the range is not empty", what, gi, k);
  auto same_record = [&](DObj a, DObj b) {
    CHECK(a.tri_begin == ga.tri_begin && a.node_begin == ga.node_begin && b.tri_begin == gb.tri_begin && b.node_begin == gb.node_begin, "%s: mesh %zu: a record does not name the mesh's ranges", what, gi);
    a.tri_begin = b.tri_begin = a.node_begin = b.node_begin = 0;
    return !memcmp(&a, &b, sizeof(DObj));
  };
  CHECK(same_record(A.objs[ga.obj_index], B.objs[gb.obj_index]), "%s: mesh %zu: objs", what, gi);
  if (ga.mesh_pos >= 0) CHECK(same_record(A.meshes[ga.mesh_pos], B.meshes[gb.mesh_pos]), "%s: mesh %zu: meshes", what, gi);
}

static void same_scene(const char *what, const FlatScene &A, const Model &m) {
  const FlatScene B = guarded(m);
  ranges_hold(what, A);
  std::vector<const Tris *> tris;
  for (const Item &it : m.items)
    if (it.o.type == CTR_OBJ_MESH) tris.push_back(&it.tris);
  CHECK(A.guards.size() == B.guards.size() && A.guards.size() == tris.size(), "%s: %zu / %zu meshes", what, A.guards.size(), B.guards.size());
  for (size_t gi = 0; gi < A.guards.size() && gi < B.guards.size() && gi < tris.size(); gi++) same_mesh(what, A, B, gi, *tris[gi]);
  // no range: byte for byte
  CHECK(same_bytes(A.planes, B.planes) && A.n_axis_recs == B.n_axis_recs, "%s: planes (%zu / %zu records, %u / %u on the axes)", what, A.planes.size(), B.planes.size(), A.n_axis_recs, B.n_axis_recs);
  CHECK(same_bytes(A.lights, B.lights) && same_bytes(A.mats, B.mats), "%s: lights or materials", what);
  CHECK(A.all_opaque == B.all_opaque && A.need_cold == B.need_cold && A.any_bounce == B.any_bounce && A.fast_pow_ok == B.fast_pow_ok && A.has_mesh == B.has_mesh, "%s: flags", what);
  CHECK(same_bytes(A.nodes, B.nodes) && A.n_mesh == B.n_mesh && A.tlas_root == B.tlas_root && A.tlas_begin == B.tlas_begin && !memcmp(A.tl_mn, B.tl_mn, 12) && !memcmp(A.tl_mx, B.tl_mx, 12),
        "%s: the top-level tree (%zu / %zu nodes, %u / %u meshes, root %#x / %#x)", what, A.nodes.size(), B.nodes.size(), A.n_mesh, B.n_mesh, A.tlas_root, B.tlas_root);
  CHECK(A.meshes.size() == A.n_mesh && !A.merged.reserved && !A.merged.built && !A.merged.usable, "%s: the merged tree is not retired", what);
  CHECK(A.mesh_tris == B.mesh_tris && A.ray_slots == B.ray_slots && A.ray_slots == ray_stack_slots(A), "%s: mesh_tris %llu / %llu, ray_slots %u / %u", what,
        (unsigned long long)A.mesh_tris, (unsigned long long)B.mesh_tris, A.ray_slots, B.ray_slots);
  CHECK(live_mesh_bytes(A) == live_mesh_bytes(B) && A.mesh_bytes == live_mesh_bytes(A), "%s: live_mesh_bytes %zu / %zu, mesh_bytes %zu", what, live_mesh_bytes(A), live_mesh_bytes(B), A.mesh_bytes);
  // objs and oloop: but for where a stand-alone triangle's record lies
  CHECK(A.objs.size() == B.objs.size() && A.objs.size() == m.items.size() && A.oloop.size() == B.oloop.size(), "%s: %zu / %zu objects, %zu / %zu in oloop", what, A.objs.size(), B.objs.size(), A.oloop.size(), B.oloop.size());
  for (size_t i = 0; i < A.oloop.size() && i < B.oloop.size(); i++) {
    DObj a = A.oloop[i], b = B.oloop[i];
    CHECK(a.index < A.objs.size() && a.tri_begin == A.objs[a.index].tri_begin, "%s: oloop %zu does not name its object's record", what, i);
    a.tri_begin = b.tri_begin = 0;
    CHECK(!memcmp(&a, &b, sizeof(DObj)), "%s: oloop %zu", what, i);
  }
  for (size_t i = 0; i < A.objs.size() && i < B.objs.size(); i++) {
    CHECK(A.objs[i].index == i, "%s: object %zu carries index %u", what, i, A.objs[i].index);
    if (A.objs[i].type == CTR_OBJ_MESH) continue;
    DObj a = A.objs[i], b = B.objs[i];
    if (a.type == CTR_OBJ_TRIANGLE && b.type == CTR_OBJ_TRIANGLE) {
      CHECK(!memcmp(&A.tris[a.tri_begin], &B.tris[b.tri_begin], sizeof(DTri)) && !memcmp(&A.gn[4 * (size_t)a.tri_begin], &B.gn[4 * (size_t)b.tri_begin], 16), "%s: object %zu: the stand-alone triangle's record", what, i);
      a.tri_begin = b.tri_begin = 0;
    }
    CHECK(!memcmp(&a, &b, sizeof(DObj)), "%s: object %zu", what, i);
  }
}

static void line(const char *what, const FlatScene &A, const Added &ad = Added()) {
  const SceneRoom r = scene_room(A);
  size_t guarded_now = 0;
  for (const MeshGuard &g : A.guards) guarded_now += g.guarded.size();
  printf("topology %-44s objects %2zu meshes %u planes %zu axis %u tris %llu/%llu nodes4 %llu/%llu reused %d %d guarded %zu\n", what, A.objs.size(), A.n_mesh, A.planes.size(), A.n_axis_recs,
         (unsigned long long)r.tris_live, (unsigned long long)r.tris_total, (unsigned long long)r.nodes4_live, (unsigned long long)r.nodes4_total, (int)ad.tris_reused, (int)ad.nodes_reused, guarded_now);
}

static void step(const char *what, const FlatScene &A, const Model &m, const Added &ad = Added()) {
  same_scene(what, A, m);
  line(what, A, ad);
}

// ---- the rows ----
static const Item NEW_SPHERE = sphere(ctr_vec3{1.5f, -2.f, 4.f}, 0.5f, GLASS);
static const Item NEW_WALL = plane(ctr_vec3{0, 0, 9}, ctr_vec3{0, 0, -1}, MIRROR);
static const Item NEW_TRI = triangle(ctr_vec3{2, -1, 5}, ctr_vec3{3, -0.5f, 5.5f}, ctr_vec3{2.5f, 1, 5}, OTHER);

static void check_room_removes() {
  const struct { const char *what; size_t i; } row[] = {{"room: remove the sphere", ROOM_SPHERE}, {"room: remove the triangle", ROOM_TRI}, {"room: remove a wall", ROOM_WALL},
                                                        {"room: remove the small mesh", ROOM_SMALL}, {"room: remove the big mesh", ROOM_MESH}};
  for (const auto &r : row) {
    Model m = room_model();
    FlatScene A = guarded(m);
    remove(A, m, r.i);
    step(r.what, A, m);
  }
  // all five on one scene, highest index first and lowest last: every index below a removed one stays, every one above moves
  Model m = room_model();
  FlatScene A = guarded(m);
  for (size_t i : {(size_t)ROOM_SPHERE, (size_t)ROOM_TRI - 1u, (size_t)ROOM_WALL - 2u, (size_t)ROOM_SMALL - 1u, (size_t)ROOM_MESH}) remove(A, m, i);
  step("room: remove all five in a row", A, m);
}

static void check_room_adds() {
  rng.seed(31);
  const Item small = mesh(shifted(guard_tris(0, 12, false), -2.5f, 1.f), OPAQUE), big = mesh(shifted(guard_tris(5, 65, false), 0.f, 1.5f), MIRROR);
  const struct { const char *what; const Item *it; } row[] = {{"room: add a sphere", &NEW_SPHERE}, {"room: add a plane", &NEW_WALL}, {"room: add a triangle", &NEW_TRI},
                                                              {"room: add a mesh of 12", &small}, {"room: add a mesh of 70", &big}};
  for (const auto &r : row) {
    Model m = room_model();
    FlatScene A = guarded(m);
    const Added ad = add(A, m, *r.it);
    CHECK(!ad.tris_reused && !ad.nodes_reused, "%s: nothing was freed, yet a range is reused", r.what);
    step(r.what, A, m, ad);
  }
  Model m = room_model();
  FlatScene A = guarded(m);
  for (const auto &r : row) add(A, m, *r.it);
  step("room: add all five in a row", A, m);
  // the far wall reflecting and at z = 0: the eye's image lies in z = 0.5, and the added mesh's five triangles there are guarded;
  // without the wall they are not
  m = room_model();
  m.items[ROOM_WALL] = plane(ctr_vec3{0, 0, 0}, ctr_vec3{0, 0, 1}, MIRROR);
  m.items.erase(m.items.begin() + ROOM_MESH);
  A = guarded(m);
  add(A, m, big);
  CHECK(A.guards.back().guarded.size() == 5 && !A.guards.back().linear, "mirror wall: %zu guarded triangles in the added mesh", A.guards.back().guarded.size());
  step("mirror wall: add a mesh with 5 in z = 0.5", A, m);
  remove(A, m, ROOM_WALL - 1u);
  CHECK(A.guards.back().guarded.empty(), "mirror wall removed: %zu guarded triangles remain", A.guards.back().guarded.size());
  step("mirror wall: remove the wall", A, m);
}

static Model one_mesh_room(const Tris &t) {
  Model m = empty_model();
  m.items.push_back(mesh(t, OPAQUE));
  for (const auto &w : WALLS) m.items.push_back(plane(w[0], w[1], OTHER));
  return m;
}

static void check_mesh_counts() {
  rng.seed(32);
  const Tris a = shifted(random_tris(70, 1.f, 0.3f), 0.f, 0.f, 3.f), b = shifted(random_tris(12, 0.6f, 0.3f), 2.5f, 0.f, 3.f);
  Model m = one_mesh_room(a);
  FlatScene A = guarded(m);
  Added ad = add(A, m, mesh(b, MIRROR));
  CHECK(A.n_mesh == 2 && !(A.tlas_root & BVH_LEAF_FLAG), "1 -> 2 meshes: n_mesh %u root %#x", A.n_mesh, A.tlas_root);
  step("meshes 1 -> 2", A, m, ad);
  remove(A, m, m.items.size() - 1);
  CHECK(A.n_mesh == 1 && (A.tlas_root & BVH_LEAF_FLAG), "2 -> 1 meshes: n_mesh %u root %#x", A.n_mesh, A.tlas_root);
  step("meshes 2 -> 1", A, m);
  remove(A, m, 0);
  CHECK(A.n_mesh == 0 && !A.has_mesh && A.nodes.empty() && A.meshes.empty(), "1 -> 0 meshes: n_mesh %u has_mesh %d", A.n_mesh, (int)A.has_mesh);
  step("meshes 1 -> 0", A, m);
  ad = add(A, m, mesh(a, OPAQUE));
  CHECK(A.n_mesh == 1 && A.has_mesh && ad.tris_reused && ad.nodes_reused, "0 -> 1 meshes: n_mesh %u reused %d %d", A.n_mesh, (int)ad.tris_reused, (int)ad.nodes_reused);
  step("meshes 0 -> 1", A, m, ad);
}

static void check_six_meshes() {
  rng.seed(33);
  Model m = empty_model();
  for (int k = 0; k < 6; k++) m.items.push_back(mesh(shifted(random_tris(12, 0.5f, 0.3f), 2.f * (float)(k % 3) - 2.f, 1.5f * (float)(k / 3), 3.f + 0.7f * (float)k), k == 4 ? MIRROR : OPAQUE));
  m.items.push_back(plane(WALLS[2][0], WALLS[2][1], OTHER));
  FlatScene A = guarded(m);
  CHECK(A.nodes.size() >= 3, "six meshes: a top-level tree of %zu nodes", A.nodes.size());
  remove(A, m, 2);
  step("six meshes: remove the third", A, m);
  const Item again = m.items[0];
  const Added ad = add(A, m, again);
  CHECK(ad.tris_reused && ad.nodes_reused, "six meshes: a mesh of 12 does not reuse the range a mesh of 12 left");
  step("six meshes: add one back", A, m, ad);
}

static void check_planes() {
  Model m = room_model();
  FlatScene A = guarded(m);
  CHECK(A.n_axis_recs == 3 && A.planes.size() == 3, "five walls: %u axis records of %zu", A.n_axis_recs, A.planes.size());
  remove(A, m, ROOM_WALL);
  step("planes 5 -> 4", A, m);
  remove(A, m, 5);
  remove(A, m, 3);
  CHECK(A.n_axis_recs == 0 && A.planes.size() == 1, "two walls: %u axis records of %zu", A.n_axis_recs, A.planes.size());
  step("planes 4 -> 2: general pairs", A, m);
  for (int w : {2, 3, 4}) add(A, m, plane(WALLS[w][0], WALLS[w][1], OTHER));
  CHECK(A.n_axis_recs == 3 && A.planes.size() == 3, "five walls again: %u axis records of %zu", A.n_axis_recs, A.planes.size());
  step("planes 2 -> 5: triples again", A, m);
  add(A, m, plane(ctr_vec3{0, 0, 7}, ctr_vec3{0.1f, 0.f, -1.f}, OTHER));
  step("planes 5 -> 6: a general one beside the triple", A, m);
}

static void check_empty() {
  rng.seed(34);
  Model m = room_model();
  FlatScene A = guarded(m);
  while (!m.items.empty()) remove(A, m, m.items.size() / 2);
  CHECK(A.objs.empty() && A.oloop.empty() && A.planes.empty() && A.meshes.empty() && A.guards.empty() && !A.has_mesh, "remove everything: something remains");
  step("remove everything", A, m);
  Added ad = add(A, m, NEW_TRI);
  CHECK(ad.tris_reused, "the triangle does not take the freed record");
  step("empty: add a triangle", A, m, ad);
  add(A, m, NEW_SPHERE);
  add(A, m, NEW_WALL);
  ad = add(A, m, mesh(shifted(guard_tris(2, 10, false), 0.f, 1.f), OPAQUE));
  CHECK(ad.tris_reused && ad.nodes_reused && ad.tri_cap == 70, "empty: a mesh of 12 takes the lowest range that fits, the big mesh's: reused %d %d tri_cap %u", (int)ad.tris_reused, (int)ad.nodes_reused, ad.tri_cap);
  step("empty: add a sphere, a plane, a mesh of 12", A, m, ad);
  // an empty mesh: created, removed
  m = empty_model();
  m.items = {mesh(Tris(), OPAQUE), sphere(ctr_vec3{0, 0, 3}, 1.f, OPAQUE), mesh(guard_tris(0, 12, false), OPAQUE)};
  A = guarded(m);
  remove(A, m, 0);
  step("remove an empty mesh", A, m);
}

static void check_steady_state() {
  rng.seed(35);
  Model m = room_model();
  FlatScene A = guarded(m);
  SceneRoom first{};
  const Tris spawned = shifted(random_tris(70, 1.f, 0.3f), 0.f, 2.f, 2.f);  // (the same triangles every round: the same tree, the same room)
  for (int round = 0; round < 8; round++) {
    const Added ad = add(A, m, mesh(spawned, round % 2 ? MIRROR : OPAQUE));
    same_scene("steady state: added", A, m);
    const SceneRoom now = scene_room(A);
    if (round == 0) first = now;
    CHECK(ad.tris_reused == (round > 0) && ad.nodes_reused == (round > 0), "round %d: reused %d %d", round, (int)ad.tris_reused, (int)ad.nodes_reused);
    CHECK(now.tris_total == first.tris_total && now.nodes4_total == first.nodes4_total, "round %d: the arrays grew to %llu and %llu records", round, (unsigned long long)now.tris_total, (unsigned long long)now.nodes4_total);
    const std::string what = "steady state: round " + std::to_string(round);
    line(what.c_str(), A, ad);
    remove(A, m, m.items.size() - 1);
    same_scene("steady state: removed", A, m);
  }
  // a freed range too small for the next mesh: appended; a smaller one takes it whole afterwards
  const size_t tris_before = A.tris.size(), nodes_before = A.nodes4.size();
  Added ad = add(A, m, mesh(shifted(random_tris(71, 1.f, 0.3f), 0.f, 2.f, 2.f), OPAQUE));
  CHECK(!ad.tris_reused && A.tris.size() == tris_before + 71 + CTR_GUARD_SLOTS && ad.tri_cap == 71, "71 after 70: reused %d, %zu records more", (int)ad.tris_reused, A.tris.size() - tris_before);
  step("a mesh of 71 after one of 70: appended", A, m, ad);
  ad = add(A, m, mesh(shifted(random_tris(30, 1.f, 0.3f), 1.f, 2.f, 2.f), OPAQUE));
  CHECK(ad.tris_reused && ad.tri_cap == 70 && A.tris.size() == tris_before + 71 + CTR_GUARD_SLOTS && A.nodes4.size() >= nodes_before, "30 after 70: reused %d tri_cap %u", (int)ad.tris_reused, ad.tri_cap);
  step("a mesh of 30 into the range of 70: whole", A, m, ad);
}

static void check_refusals() {
  const FlatScene A = guarded(room_model());
  std::string err;
  ctr_object o = NEW_SPHERE.o;
  o.type = CTR_OBJ_MESH;
  CHECK(check_new_object(A, o, err) == CTR_E_INVALID && err.find("ctr_scene_add_mesh") != std::string::npos, "a mesh through add_object: %s", err.c_str());
  o.type = CTR_OBJ_SPHERE + 1;
  CHECK(check_new_object(A, o, err) == CTR_E_INVALID && err.find("bad type") != std::string::npos, "type 4: %s", err.c_str());
  o = NEW_SPHERE.o;
  o.mat_idx = 4;
  CHECK(check_new_object(A, o, err) == CTR_E_INVALID && err.find("material") != std::string::npos, "material 4 of 4: %s", err.c_str());
  printf("refusals: hold\n");
}

int main() {
  check_room_removes();
  check_room_adds();
  check_mesh_counts();
  check_six_meshes();
  check_planes();
  check_empty();
  check_steady_state();
  check_refusals();
  printf(fails ? "topology_check: %d FAILURES\n" : "topology_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
