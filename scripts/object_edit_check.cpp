// object_edit_check.cpp — the host half of the object edits (include/cutrace_objects.h) without a device; meant to run under
// ASan/UBSan as well.  tests/test_object_edit_cpu.py builds and runs it (no arguments) and reads the lines it prints.
//
// Three small scenes built here — (a) four planes, two spheres and two stand-alone triangles, no mesh; (b) a box room of five
// axis-aligned planes with a 70-triangle mesh, a 12-triangle mesh, a sphere and a stand-alone triangle; (c) two meshes, a
// floor and a sphere — go through a row of edits, (b) and (c) once more with the merged tree built.  Each edit is applied to
// ONE FlatScene as ctr_scene_set_objects applies it (check_objects, objects_edited, then plan_guards / apply_guards) and
// compared with flatten_scene of the EDITED description + the guard: every array, flag and count (n_axis_recs included),
// every MeshGuard::guarded / linear and the merged tree's guard keys, byte for byte.  That comparison is the proof that nothing
// else caches an analytic object's parameter or a material index.  (Not compared, as in scene_edit_check.cpp: guard records
// and spare nodes beyond what is currently guarded.)  After each edit object_of of every object, fed back, must change nothing.
// The row runs a second time after the 70-triangle mesh went through mesh_updated (both sides: the fresh scene gets the same
// update), where the mesh's refitted box must survive every edit; light_records / material_records are interleaved; and every
// rejection of check_objects must leave the FlatScene byte-identical.
// Before the rows: plane_records_at_most, the room ctr_scene_set_objects gives the device's plane array, against flatten_scene for
// every spread of 1 .. 9 planes over the three axes and the general records.
//   bound <P> planes | worst packing <records> records | at most <bound>
//   edit <scene> | <step> | planes <records> axis <n_axis_recs> guarded <triangles> linear <meshes> mirrors <count>
//   reject <scene> | <what> | untouched
#include <algorithm>

#include "edit_check_common.h"

// material indices every scene here has
enum { OPAQUE = 0, OTHER = 1, GLASS = 2, MIRROR = 3 };

// what ctr_scene_set_objects does to the host copy: every check before the first write, the records, the guard
static int set_objects(FlatScene &F, const std::vector<DCam> &cams, const ctr_object *objects, uint64_t n, std::string &err) {
  if (int st = check_objects(F, objects, n, err)) return st;
  objects_edited(F, objects, n);
  guard(F, cams);
  return CTR_OK;
}

// every byte of every array, the records nothing reads included: a rejected edit may not have written anything
static bool identical(const FlatScene &A, const FlatScene &B) {
  return same_bytes(A.objs, B.objs) && same_bytes(A.oloop, B.oloop) && same_bytes(A.meshes, B.meshes) && same_bytes(A.planes, B.planes) &&
         same_bytes(A.tris, B.tris) && same_bytes(A.nodes, B.nodes) && same_bytes(A.nodes4, B.nodes4) && same_bytes(A.gn, B.gn) &&
         same_bytes(A.lights, B.lights) && same_bytes(A.mats, B.mats) && A.n_axis_recs == B.n_axis_recs;
}

struct Row {
  std::string name;
  Scene s;          // the description, edited step by step
  FlatScene A;      // the one flat scene every edit goes into
  bool merge = false;
  int updated = -1;  // guards[] index of the mesh that went through mesh_updated, with these triangles
  Tris new_tris;
  float box[6] = {0, 0, 0, 0, 0, 0};  // ... and its refitted box

  std::vector<DCam> cams() const { return cams_of(s.desc); }

  // a handle's life restated on a fresh flat scene of the current description
  FlatScene fresh() const {
    FlatScene B = flat_of(s.desc);
    guard(B, cams());
    if (merge && !build_merged_tree(B).empty()) guard(B, cams());
    if (updated >= 0) {
      update_on_host(B, (size_t)updated, new_tris);
      guard(B, cams());
    }
    return B;
  }

  size_t guarded() const {
    size_t n = 0;
    for (const MeshGuard &g : A.guards) n += g.guarded.size();
    return n;
  }

  void compare(const std::string &what) {
    const FlatScene B = fresh();
    same_flat(name + ": " + what, A, B);
    CHECK(A.planes.size() <= plane_records_at_most(A), "%s: %s: %zu plane records, at most %zu", name.c_str(), what.c_str(), A.planes.size(), plane_records_at_most(A));
    if (updated >= 0) {
      const DObj &O = A.objs[A.guards[updated].obj_index];
      const ctr_object back = object_of(A, A.guards[updated].obj_index);
      CHECK(!memcmp(O.f, box, sizeof(box)) && !memcmp(&back.v0, box, 12) && !memcmp(&back.v1, box + 3, 12), "%s: %s: the refitted box did not survive", name.c_str(), what.c_str());
    }
    // object_of of every object, fed back: accepted, and an identity edit
    std::vector<ctr_object> got;
    for (size_t i = 0; i < A.objs.size(); i++) got.push_back(object_of(A, i));
    FlatScene C = A;
    std::string err;
    CHECK(set_objects(C, cams(), got.data(), got.size(), err) == CTR_OK, "%s: %s: object_of fed back: %s", name.c_str(), what.c_str(), err.c_str());
    CHECK(identical(C, A), "%s: %s: object_of fed back changed something", name.c_str(), what.c_str());
    for (size_t i = 0; i < got.size(); i++)
      CHECK(got[i].type == s.objects[i].type && got[i].mat_idx == s.objects[i].mat_idx && got[i].tri_begin == 0 &&
            (got[i].type != CTR_OBJ_MESH || got[i].tri_count == s.objects[i].tri_count), "%s: %s: object_of #%zu", name.c_str(), what.c_str(), i);
    size_t linear = 0;
    for (const MeshGuard &g : A.guards) linear += g.linear;
    printf("edit %s | %s | planes %zu axis %u guarded %zu linear %zu mirrors %zu\n", name.c_str(), what.c_str(), A.planes.size(), A.n_axis_recs, guarded(), linear,
           guard_probes(A, cams()).n_mirrors);
  }

  // the three kinds of step: the description has been edited already
  void E(const std::string &what) {
    s.finish();
    std::string err;
    CHECK(set_objects(A, cams(), s.desc.objects, s.desc.n_objects, err) == CTR_OK, "%s: %s: rejected: %s", name.c_str(), what.c_str(), err.c_str());
    compare(what);
  }
  void L(const std::string &what) {
    s.finish();
    light_records(A, s.desc.lights, s.desc.n_lights);
    guard(A, cams());
    compare(what);
  }
  void M(const std::string &what) {
    s.finish();
    material_records(A, s.desc.materials, s.desc.n_materials);
    guard(A, cams());
    compare(what);
  }

  // must be rejected, with A untouched
  void R(const char *what, const ctr_object *objects, uint64_t n, const char *text) {
    const FlatScene before = A;
    std::string err;
    const int st = set_objects(A, cams(), objects, n, err);
    CHECK(st == CTR_E_INVALID && err.find(text) != std::string::npos, "%s: %s: status %d, \"%s\"", name.c_str(), what, st, err.c_str());
    CHECK(identical(A, before) && A.guards.size() == before.guards.size(), "%s: %s: the rejected edit wrote something", name.c_str(), what);
    for (size_t i = 0; i < A.guards.size() && i < before.guards.size(); i++)
      CHECK(A.guards[i].guarded == before.guards[i].guarded && A.guards[i].linear == before.guards[i].linear, "%s: %s: guard state", name.c_str(), what);
    if (st == CTR_E_INVALID && identical(A, before)) printf("reject %s | %s | untouched\n", name.c_str(), what);
  }

  std::vector<size_t> of_type(uint32_t type) const {
    std::vector<size_t> ids;
    for (size_t i = 0; i < s.objects.size(); i++)
      if (s.objects[i].type == type) ids.push_back(i);
    return ids;
  }
};

static ctr_vec3 plus(ctr_vec3 a, float x, float y, float z) { return ctr_vec3{a.x + x, a.y + y, a.z + z}; }

// the row every scene goes through; `tag` distinguishes its second pass (after the mesh update)
static void edits(Row &r, const std::string &tag) {
  Scene &s = r.s;
  const std::vector<ctr_object> objects0 = s.objects;
  auto E = [&](const std::string &what) { r.E(tag + what); };
  E("nothing changed");
  // ---- spheres ----
  for (size_t i : r.of_type(CTR_OBJ_SPHERE)) {
    const std::string w = "sphere #" + std::to_string(i);
    s.objects[i].v0 = plus(s.objects[i].v0, 0.37f, -0.21f, 0.11f);
    E(w + " moved");
    s.objects[i].f0 *= 1.7f;
    E(w + " resized");
    s.objects[i].f0 = 0.f;
    E(w + " radius 0");
    s.objects[i].f0 = -0.5f;
    E(w + " radius -0.5");
    s.objects[i] = objects0[i];
    E(w + " back");
  }
  // ---- stand-alone triangles ----
  for (size_t i : r.of_type(CTR_OBJ_TRIANGLE)) {
    const std::string w = "triangle #" + std::to_string(i);
    s.objects[i].v0 = plus(s.objects[i].v0, 0.3f, 0.1f, -0.2f);
    s.objects[i].v1 = plus(s.objects[i].v1, -0.1f, 0.25f, 0.15f);
    s.objects[i].v2 = plus(s.objects[i].v2, 0.2f, -0.3f, 0.4f);
    E(w + " three points moved");
    s.objects[i].v2 = s.objects[i].v1;
    E(w + " of no area");
    s.objects[i] = objects0[i];
    E(w + " back");
  }
  // ---- planes: the packing ----
  const std::vector<size_t> planes = r.of_type(CTR_OBJ_PLANE);
  auto tilt = [&](size_t i) {  // a second normal component: off its axis
    ctr_vec3 &n = s.objects[i].v1;
    (n.x != 0.f ? n.y : n.x) = 0.25f;
  };
  if (!planes.empty()) {
    const size_t p = planes[0];
    const std::string w = "plane #" + std::to_string(p);
    tilt(p);
    E(w + " tilted off its axis");
    s.objects[p] = objects0[p];
    E(w + " back on its axis");
    s.objects[p].v0 = plus(s.objects[p].v0, 0.4f, -0.3f, 0.2f);
    E(w + " point moved");
    s.objects[p].v0.y = 2e37f;
    E(w + " point beyond 1e37");
    s.objects[p].v0 = ctr_vec3{-3e38f, 0.f, INFINITY};
    E(w + " point at infinity");
    s.objects[p] = objects0[p];
    ctr_vec3 &n = s.objects[p].v1;
    for (float *c : {&n.x, &n.y, &n.z})
      if (*c == 0.f) *c = -0.0f;
    E(w + " normal with -0.0 components");
    n = ctr_vec3{0.f, 0.f, 0.f};
    E(w + " zero normal");
    n = ctr_vec3{-0.0f, 0.f, -0.0f};
    E(w + " zero normal with -0.0");
    s.objects[p] = objects0[p];
    E(w + " back");
    // all but two planes tilted: fewer than three axis-aligned ones flip the WHOLE array to general pairs
    for (size_t k = 2; k < planes.size(); k++) tilt(planes[k]);
    E("all but two planes tilted");
    for (size_t k = 2; k < planes.size(); k++) s.objects[planes[k]] = objects0[planes[k]];
    E("the planes back on their axes");
    // every plane onto ONE axis, then the last of them general beside the others: whichever needs more records is the most the
    // scene can need (plane_records_at_most; for an even number of planes the second, one more than the first)
    size_t most = 0;
    for (size_t k : planes) s.objects[k].v1 = ctr_vec3{0.f, 1.f, 0.f};
    E("every plane normal to y");
    most = std::max(most, r.A.planes.size());
    s.objects[planes.back()].v1 = ctr_vec3{0.25f, 1.f, 0.f};
    E("every plane normal to y but the last, which is general");
    most = std::max(most, r.A.planes.size());
    CHECK(planes.size() < 4 || most == plane_records_at_most(r.A), "%s: %zu records at the worst packing, at most %zu", r.name.c_str(), most, plane_records_at_most(r.A));
    // ... reached from general pairs alone, the fewest records: the largest growth one edit can ask of the device array
    for (size_t k : planes) s.objects[k].v1 = ctr_vec3{0.25f, 1.f, 0.125f};
    E("every plane general");
    for (size_t k : planes) s.objects[k].v1 = ctr_vec3{0.f, 1.f, 0.f};
    s.objects[planes.back()].v1 = ctr_vec3{0.25f, 1.f, 0.f};
    E("from general pairs to every plane normal to y but the last");
    for (size_t k : planes) s.objects[k] = objects0[k];
    E("the planes as they were");
  }
  // ---- material indices: every object opaque -> transparent -> opaque, not reflecting -> reflecting -> back ----
  for (size_t i = 0; i < s.objects.size(); i++) {
    const std::string w = "object #" + std::to_string(i) + " (type " + std::to_string(s.objects[i].type) + ")";
    s.objects[i].mat_idx = GLASS;
    E(w + " transparent");
    s.objects[i].mat_idx = OTHER;
    E(w + " opaque");
    s.objects[i].mat_idx = MIRROR;
    E(w + " reflecting");
    s.objects[i].mat_idx = objects0[i].mat_idx;
    E(w + " its own material again");
  }
  for (ctr_object &o : s.objects) o.mat_idx = GLASS;
  E("everything transparent");
  s.objects = objects0;
  E("everything as it was");
}

// scene (b) only: wall `wall` (normal to z) becomes a mirror and moves so that the eye's image lies in z = 0.5, the plane of five
// triangles of the first mesh, and out again
static void moving_mirror(Row &r, size_t wall, const std::string &tag) {
  Scene &s = r.s;
  const ctr_object wall0 = s.objects[wall];
  const size_t before = r.guarded();
  s.objects[wall].mat_idx = MIRROR;
  r.E(tag + "the wall reflects");
  CHECK(r.guarded() == before, "%s: %sthe wall reflects: %zu guarded", r.name.c_str(), tag.c_str(), r.guarded());
  s.objects[wall].v0.z = 0.f;  // the eye at z = -0.5: its image at z = 0.5
  r.E(tag + "the mirror moved: the eye's image in z = 0.5");
  CHECK(r.guarded() == before + 5, "%s: %sthe mirror moved: %zu guarded, %zu before", r.name.c_str(), tag.c_str(), r.guarded(), before);
  s.objects[wall].v0.z = wall0.v0.z;
  r.E(tag + "the mirror moved back");
  CHECK(r.guarded() == before, "%s: %sthe mirror moved back: %zu guarded", r.name.c_str(), tag.c_str(), r.guarded());
  s.objects[wall] = wall0;
  r.E(tag + "the wall reflects no more");
}

// with the other edits in between
static void interleaved(Row &r) {
  Scene &s = r.s;
  const std::vector<ctr_object> objects0 = s.objects;
  const std::vector<ctr_light> lights0 = s.lights;
  const std::vector<ctr_material> mats0 = s.materials;
  s.materials[OTHER].transparency = 0.4f;
  r.M("material 1 transmits");
  for (ctr_object &o : s.objects) o.mat_idx = o.mat_idx == OTHER ? OPAQUE : OTHER;
  r.E("materials 0 and 1 swapped on every object");
  s.lights.assign(1, light(CTR_LIGHT_POINT, 3.f, -1.f, 0.5f));
  r.L("a point light in z = 0.5");
  for (size_t i : r.of_type(CTR_OBJ_SPHERE)) s.objects[i].v0 = plus(s.objects[i].v0, 0.f, 0.5f, 0.f);
  r.E("the spheres raised");
  s.materials.push_back(material(0.6f, 0.f, 20.f));
  r.M("one material more, reflecting");
  for (size_t i : r.of_type(CTR_OBJ_PLANE)) s.objects[i].mat_idx = s.materials.size() - 1;
  r.E("every plane takes the new material");
  s.objects = objects0;
  r.E("the first objects again");
  s.materials = mats0;
  r.M("the first materials again");
  s.lights = lights0;
  r.L("the first lights again");
}

static void rejections(Row &r) {
  const Scene &s = r.s;
  const uint64_t n = s.objects.size();
  std::vector<ctr_object> o = s.objects;
  r.R("null objects", nullptr, n, "null argument");
  r.R("one object fewer", o.data(), n - 1, "the count is fixed");
  o.push_back(o[0]);
  r.R("one object more", o.data(), n + 1, "the count is fixed");
  o = s.objects;
  o.back().type = CTR_OBJ_SPHERE + 1;
  r.R("a type above the last", o.data(), n, "bad type");
  o = s.objects;
  o[0].type = o[0].type == CTR_OBJ_PLANE ? CTR_OBJ_SPHERE : CTR_OBJ_PLANE;
  o[1].v0 = plus(o[1].v0, 1.f, 1.f, 1.f);  // (valid, and after the bad one: not written either)
  r.R("another type", o.data(), n, "the type is fixed");
  o = s.objects;
  o[0].v0 = plus(o[0].v0, 1.f, 1.f, 1.f);  // (valid, and BEFORE the bad one: every check runs before the first write)
  o.back().mat_idx = s.materials.size();
  r.R("a material index one past the last", o.data(), n, "material index out of range");
  o.back().mat_idx = (1ull << 32) | 1u;
  r.R("a material index beyond 32 bits", o.data(), n, "material index out of range");
  for (size_t i : r.of_type(CTR_OBJ_MESH)) {
    o = s.objects;
    o[0].v0 = plus(o[0].v0, 1.f, 1.f, 1.f);
    o[i].tri_count += 1;
    r.R("a mesh with one triangle more", o.data(), n, "the count is fixed");
    o[i].tri_count = 0;
    r.R("a mesh with no triangle", o.data(), n, "the count is fixed");
  }
}

static void run(const std::string &name, const Scene &scene, bool merge, int wall, int update_mesh) {
  Row r;
  r.name = name + (merge ? " (merged)" : "");
  r.s = Scene::copy_of(scene.desc);
  r.merge = merge;
  r.A = r.fresh();
  const ctr_scene_desc d0 = scene.desc;
  edits(r, "");
  if (wall >= 0) moving_mirror(r, (size_t)wall, "");
  interleaved(r);
  rejections(r);
  if (update_mesh >= 0) {
    // the mesh's triangles slide within their planes; from here on both sides hold a refitted tree and box
    const ctr_object &o = r.s.objects[r.A.guards[update_mesh].obj_index];
    r.new_tris.assign(r.s.triangles.begin() + o.tri_begin, r.s.triangles.begin() + o.tri_begin + o.tri_count);
    for (ctr_triangle &t : r.new_tris)
      for (ctr_vec3 *p : {&t.p1, &t.p2, &t.p3}) { p->x += 0.125f; p->y -= 0.0625f; }
    update_on_host(r.A, (size_t)update_mesh, r.new_tris);
    guard(r.A, r.cams());
    r.updated = update_mesh;
    memcpy(r.box, r.A.objs[r.A.guards[update_mesh].obj_index].f, sizeof(r.box));
    CHECK(memcmp(r.box, &o.v0, 12) != 0, "%s: the update did not move the mesh's box", r.name.c_str());
    r.compare("after mesh_updated");
    edits(r, "updated: ");
    if (wall >= 0) moving_mirror(r, (size_t)wall, "updated: ");
    interleaved(r);
    rejections(r);
  }
  const FlatScene B = r.fresh();
  CHECK(r.s.objects.size() == d0.n_objects && !memcmp(r.s.objects.data(), d0.objects, d0.n_objects * sizeof(ctr_object)), "%s: the description is not back where it started", r.name.c_str());
  same_flat(r.name + ": back where it started", r.A, B);
}

static Scene with_materials() {
  Scene s;
  s.materials = {material(0.f, 0.f, 40.f), material(0.f, 0.f, 10.f), material(0.f, 0.5f, 20.f), material(0.4f, 0.f, 30.f)};
  s.lights = {light(CTR_LIGHT_POINT, 3.f, -1.f, 1.f), light(CTR_LIGHT_SUN, 0.3f, -0.8f, 0.5f)};
  s.cam.pos = ctr_vec3{0.3f, 0.2f, -0.5f};
  s.cam.w = s.cam.h = 16;
  return s;
}

// plane_records_at_most against flatten_scene itself: every way to spread 1 .. 9 planes over the three axes and the general
// records; no packing may need more records than the bound, and some packing must need exactly that many
static void check_bound() {
  for (size_t P = 1; P <= 9; P++) {
    size_t most = 0, bound = 0;
    for (size_t x = 0; x <= P; x++)
      for (size_t y = 0; x + y <= P; y++)
        for (size_t z = 0; x + y + z <= P; z++) {
          Scene s = with_materials();
          for (size_t k = 0; k < P; k++) {
            const ctr_vec3 n = k < x ? ctr_vec3{1, 0, 0} : k < x + y ? ctr_vec3{0, -1, 0} : k < x + y + z ? ctr_vec3{0, 0, 2} : ctr_vec3{0.5f, 1, 0};
            s.plane(ctr_vec3{0.f, -1.f - (float)k, 0.f}, n, OPAQUE);
          }
          s.finish();
          const FlatScene F = flat_of(s.desc);
          bound = plane_records_at_most(F);
          CHECK(F.planes.size() <= bound, "bound: %zu planes (%zu, %zu, %zu on the axes): %zu records, at most %zu", P, x, y, z, F.planes.size(), bound);
          most = std::max(most, F.planes.size());
        }
    CHECK(most == bound, "bound: %zu planes: the worst packing needs %zu records, plane_records_at_most says %zu", P, most, bound);
    printf("bound %zu planes | worst packing %zu records | at most %zu\n", P, most, bound);
  }
}

int main() {
  check_bound();
  {  // (a) no mesh: a floor, a tilted plane, two walls; two spheres, two stand-alone triangles
    Scene s = with_materials();
    s.plane(ctr_vec3{0, -1, 0}, ctr_vec3{0, 1, 0}, OTHER);
    s.sphere(ctr_vec3{0.f, 0.f, 3.f}, 0.8f, OPAQUE);
    s.plane(ctr_vec3{0, 0, 9}, ctr_vec3{0.2f, 0.1f, -1.f}, OPAQUE);
    s.triangle(ctr_vec3{-1, 0, 4}, ctr_vec3{1, 0.5f, 4.5f}, ctr_vec3{0, 2, 4}, OTHER);
    s.plane(ctr_vec3{-4, 0, 0}, ctr_vec3{1, 0, 0}, OPAQUE);
    s.sphere(ctr_vec3{1.5f, 0.5f, 2.f}, 0.4f, OTHER);
    s.triangle(ctr_vec3{2, -1, 5}, ctr_vec3{3, 1, 5}, ctr_vec3{2.5f, 1.5f, 6}, OPAQUE);
    s.plane(ctr_vec3{4, 0, 0}, ctr_vec3{-1, 0, 0}, OTHER);
    s.finish();
    run("a: planes, spheres, triangles", s, false, -1, -1);
  }
  {  // (b) the box room: five axis-aligned walls (the fifth, normal to z, is the one that becomes the moving mirror)
    Scene s = with_materials();
    s.plane(ctr_vec3{-5, 0, 0}, ctr_vec3{1, 0, 0}, OTHER);
    s.plane(ctr_vec3{5, 0, 0}, ctr_vec3{-1, 0, 0}, OTHER);
    s.mesh(guard_tris(5, 65, false), OPAQUE);  // 70 triangles, five of them in z = 0.5
    s.plane(ctr_vec3{0, -3, 0}, ctr_vec3{0, 1, 0}, OTHER);
    s.sphere(ctr_vec3{-2.f, -1.f, 3.f}, 0.7f, OPAQUE);
    s.plane(ctr_vec3{0, 8, 0}, ctr_vec3{0, -1, 0}, OTHER);
    Tris small = guard_tris(0, 12, false);  // 12 triangles: a mesh small enough for each of them to be a mirror
    for (ctr_triangle &t : small)
      for (ctr_vec3 *p : {&t.p1, &t.p2, &t.p3}) p->x += 2.5f;
    s.mesh(small, MIRROR);
    s.triangle(ctr_vec3{-3, 0, 6}, ctr_vec3{-2, 0.5f, 6.5f}, ctr_vec3{-2.5f, 2, 6}, OPAQUE);
    s.plane(ctr_vec3{0, 0, -6}, ctr_vec3{0, 0, 1}, OTHER);
    s.finish();
    const int wall = (int)s.objects.size() - 1;
    run("b: box room", s, false, wall, 0);
    run("b: box room", s, true, wall, 0);
  }
  {  // (c) two meshes: the merged tree has its room reserved
    Scene s = with_materials();
    s.mesh(guard_tris(3, 40, false), OPAQUE);
    s.plane(ctr_vec3{0, -2, 0}, ctr_vec3{0, 1, 0}, OTHER);
    Tris second = guard_tris(2, 30, false);
    for (ctr_triangle &t : second)
      for (ctr_vec3 *p : {&t.p1, &t.p2, &t.p3}) p->x += 0.4f;
    s.mesh(second, OTHER);
    s.sphere(ctr_vec3{1.f, 0.f, -3.f}, 0.5f, OPAQUE);
    s.finish();
    FlatScene F = flat_of(s.desc);
    CHECK(F.merged.reserved, "c: the merged tree is not reserved");
    run("c: two meshes", s, false, -1, -1);
    run("c: two meshes", s, true, -1, -1);
  }
  printf(fails ? "object_edit_check: %d FAILURES\n" : "object_edit_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
