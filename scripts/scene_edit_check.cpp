// scene_edit_check.cpp — the host-checkable half of the light and material edits (include/cutrace_edit.h) without a device; meant to
// run under ASan/UBSan as well.  tests/test_scene_edit_cpu.py builds and runs it (arguments: scene files, read by the host loader
// from the current directory) and reads the lines it prints.
//
//   edit     Over the scene files and small guard scenes built here: flatten_scene + the guard, then a row of edits through
//            light_records / material_records (scene_flatten.h) + plan_guards / apply_guards, each against flatten_scene of the
//            EDITED description + the guard: every array, every flag, every MeshGuard::guarded / linear and — where the scene has
//            one — the merged tree's guard keys, byte for byte.  (Not compared, because nothing reads them: guard records and
//            spare nodes beyond what is currently guarded keep what an earlier guard state left there.)  The edits flip every
//            flag both ways; the line of a step names the flags.
//   scan     guard_scan.h compiled for the host, turned into bit words and cut at each mesh's range exactly as the device
//            path's host half does, against the loop guard.cpp had before the two were split (kept here as the yardstick):
//            mesh sizes 1, 63, 64, 65, 257 and two meshes of 65 and 64 (the second range starts inside a word), in-plane
//            triangles at leaf positions 0, 63, 64 and n - 1, 64 and 65 of them, zero-area triangles, suns, no light at all.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "bvh.h"
#include "cutrace_host.h"
#include "guard.h"
#include "guard_scan.h"
#include "scene_flatten.h"

#include "edit_check_common.h"

// one edit: `s` has been edited already; A follows through the shared functions, B is flattened anew
static void step(const std::string &scene, const char *what, const Scene &s, FlatScene &A, bool lights, bool merge) {
  const std::vector<DCam> cams = cams_of(s.desc);
  if (lights) light_records(A, s.desc.lights, s.desc.n_lights);
  else material_records(A, s.desc.materials, s.desc.n_materials);
  guard(A, cams);
  FlatScene B = flat_of(s.desc);
  guard(B, cams);
  if (merge && !build_merged_tree(B).empty()) guard(B, cams);
  same_flat(scene + ": " + what, A, B);
  size_t guarded = 0, linear = 0;
  for (const MeshGuard &g : A.guards) { guarded += g.guarded.size(); linear += g.linear; }
  printf("edit %s | %s | all_opaque %d need_cold %d any_bounce %d fast_pow_ok %d guarded %zu linear %zu merged_keys %zu\n", scene.c_str(), what,
         (int)A.all_opaque, (int)A.need_cold, (int)A.any_bounce, (int)A.fast_pow_ok, guarded, linear, A.merged.built && A.merged.usable ? A.merged.guarded.size() : 0);
}

// the row of edits every scene goes through.  Needs at least one material; works with any number of lights.
static void edit_row(const std::string &name, const ctr_scene_desc &d0, bool merge) {
  Scene s = Scene::copy_of(d0);
  const std::vector<ctr_light> lights0 = s.lights;
  const std::vector<ctr_material> mats0 = s.materials;
  FlatScene A = flat_of(s.desc);
  guard(A, cams_of(s.desc));
  if (merge && !build_merged_tree(A).empty()) guard(A, cams_of(s.desc));
  auto L = [&](const char *what) { s.finish(); step(name, what, s, A, true, merge); };
  auto M = [&](const char *what) { s.finish(); step(name, what, s, A, false, merge); };
  L("nothing changed");
  // ---- lights ----
  if (!s.lights.empty()) {
    s.lights[0].v = ctr_vec3{s.lights[0].v.x + 0.37f, s.lights[0].v.y - 0.21f, s.lights[0].v.z + 0.11f};
    L("light 0 moved");
    s.lights[0].color = ctr_vec3{0.f, 0.f, 0.f};
    if (s.lights.size() > 1) s.lights[1].color = ctr_vec3{-0.2f, 0.4f, 0.1f};
    L("colours 0 and negative");
    for (ctr_light &l : s.lights) l.type = l.type == CTR_LIGHT_POINT ? CTR_LIGHT_SUN : CTR_LIGHT_POINT;
    L("points and suns swapped");
  }
  s.lights.clear();
  L("no light");
  for (int k = 0; k < 5; k++) s.lights.push_back(light(k % 3 == 2 ? CTR_LIGHT_SUN : CTR_LIGHT_POINT, U(-3, 3), U(2, 6), U(-3, 3), 0.2f));
  L("five lights");
  for (int k = 5; k < 33; k++) s.lights.push_back(light(k % 3 == 2 ? CTR_LIGHT_SUN : CTR_LIGHT_POINT, U(-3, 3), U(2, 6), U(-3, 3), 0.03f));
  L("33 lights");
  s.lights.assign(1, light(CTR_LIGHT_POINT, 3.f, -1.f, 0.5f));
  L("a point light in z = 0.5");
  s.lights.assign(1, light(CTR_LIGHT_SUN, 0.3f, -0.8f, 0.f));
  L("a sun parallel to z = 0.5");
  s.lights = lights0;
  L("the first lights again");
  // ---- materials: every flag both ways ----
  for (ctr_material &m : s.materials) { m.transparency = 0.f; m.reflexivity = 0.f; m.phong_exp = 10.f; }
  M("all opaque, none reflects");
  s.materials[0].transparency = 0.4f;
  M("material 0 transmits");
  s.materials[0].reflexivity = 0.3f;
  M("material 0 transmits and reflects");
  s.materials[0].transparency = 0.f;
  M("material 0 reflects");
  s.materials[0].reflexivity = 5e-7f;
  M("material 0 reflects 5e-7");
  s.materials[0].reflexivity = 0.f;
  s.materials[0].transparency = 1e-7f;
  M("material 0 transmits 1e-7");
  s.materials[0].transparency = 0.f;
  s.materials.back().reflexivity = 0.3f;
  M("the last material reflects");
  s.materials.back().reflexivity = 0.f;
  M("all opaque, none reflects again");
  s.lights.assign(1, light(CTR_LIGHT_POINT, 1.5f, 2.5f, 2.f, 1.0f));
  L("one light of colour 1");
  s.materials[0].specular = 0.5f;
  s.materials[0].color = ctr_vec3{1.f, 1.f, 1.f};
  s.materials[0].phong_exp = 5000.f;
  M("phong exponent 5000");
  s.materials[0].phong_exp = 40.f;
  M("phong exponent 40");
  s.lights[0].color = ctr_vec3{0.f, -300.f, 0.f};
  L("light colour -300");
  s.lights[0].color = ctr_vec3{1.f, 1.f, 1.f};
  L("light colour 1");
  s.materials.push_back(material(0.5f, 0.5f, 20.f));
  M("one material more");
  s.materials.pop_back();
  M("one material fewer");
  s.materials = mats0;
  M("the first materials again");
  s.lights = lights0;
  L("the first lights again, at the end");
  FlatScene B = flat_of(d0);
  guard(B, cams_of(d0));
  if (merge && !build_merged_tree(B).empty()) guard(B, cams_of(d0));
  same_flat(name + ": back where it started", A, B);
}

static void check_edits(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    ctr_host_scene *hs = nullptr;
    ctr_host_scene_load(argv[i], &hs);
    if (!hs) { printf("FAIL cannot read %s\n", argv[i]); fails++; continue; }
    const ctr_scene_desc *d = ctr_host_scene_desc(hs);
    if (d->n_materials) {
      edit_row(argv[i], *d, false);
      edit_row(std::string(argv[i]) + " (merged)", *d, true);
    }
    ctr_host_scene_free(hs);
  }
  // the small guard scenes: the eye off every plane, a floor whose image of the eye lies in z = 0.5 when it reflects
  for (size_t k : {3u, 70u}) {
    Scene s;
    s.materials = {material(0.f, 0.f, 40.f), material(0.f, 0.f, 10.f)};
    s.lights = {light(CTR_LIGHT_POINT, 3.f, -1.f, 1.f)};
    s.mesh(guard_tris(k, 400), 0);
    s.plane(ctr_vec3{0, 0, 0}, ctr_vec3{0, 0, 2.f}, 1);  // the eye (0.3, 0.2, -0.5) has its image in z = 0.5
    s.mesh(guard_tris(2, 30), 0);
    s.cam.pos = ctr_vec3{0.3f, 0.2f, -0.5f};
    s.cam.w = s.cam.h = 16;
    s.finish();
    edit_row("guard scene, " + std::to_string(k) + " in the plane", s.desc, false);
    edit_row("guard scene, " + std::to_string(k) + " in the plane (merged)", s.desc, true);
  }
}

// ---- the scan: the loop of guard.cpp before the split, kept as the yardstick ----
namespace yardstick {
constexpr double TOL = 1.0 / 131072.0;
struct P3 { double x, y, z; };
std::vector<uint32_t> risky_triangles(const MeshGuard &g, const std::vector<P3> &origins, const std::vector<DLight> &lights) {
  std::vector<uint32_t> risky;
  const size_t nt = g.planes.size() / 7;
  for (size_t t = 0; t < nt; t++) {
    const double *q = &g.planes[7 * t];
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0) continue;  // zero-area triangle: alpha is exactly 0, never a hit
    auto point_in_plane = [&](double x, double y, double z) {
      const double dx = x - q[3], dy = y - q[4], dz = z - q[5];
      const double dist = fabs(dx * q[0] + dy * q[1] + dz * q[2]);
      const double scale = fmax(fmax(fabs(dx), fabs(dy)), fmax(fabs(dz), q[6]));
      return dist <= TOL * scale;
    };
    bool hit = false;
    for (const P3 &o : origins)
      if (point_in_plane(o.x, o.y, o.z)) hit = true;
    for (const DLight &l : lights) {
      if (l.type == CTR_LIGHT_POINT) {
        if (point_in_plane(l.vx, l.vy, l.vz)) hit = true;
      } else {
        const double len = sqrt((double)l.vx * l.vx + (double)l.vy * l.vy + (double)l.vz * l.vz);
        if (len > 0.0 && fabs(l.vx * q[0] + l.vy * q[1] + l.vz * q[2]) <= TOL * len) hit = true;
      }
    }
    if (hit) risky.push_back((uint32_t)t);
  }
  return risky;
}
}  // namespace yardstick

// the scene's planes through both scans; returns the risky count per mesh
static std::vector<size_t> scan_both(const std::string &what, const FlatScene &F, const std::vector<DCam> &cams) {
  const GuardProbes P = guard_probes(F, cams);
  std::vector<yardstick::P3> origins;
  for (size_t i = 0; i < P.n_origins; i++) origins.push_back({P.probes[i].x, P.probes[i].y, P.probes[i].z});
  CHECK(P.probes.size() == P.n_origins + F.lights.size() && P.n_origins <= P.n_points && P.n_points <= P.probes.size(), "%s: %zu probes (%zu points) for %zu origins and %zu lights",
        what.c_str(), P.probes.size(), P.n_points, P.n_origins, F.lights.size());
  // the flat array and its words, as the device path builds them
  std::vector<double> flat;
  for (const MeshGuard &g : F.guards) flat.insert(flat.end(), g.planes.begin(), g.planes.end());
  const uint64_t n = guard_plane_count(F);
  CHECK(n * CTR_PLANE_DOUBLES == flat.size(), "%s: plane count", what.c_str());
  std::vector<uint64_t> words(guard_scan_words(n) + 1, 0xDEADBEEFDEADBEEFull);
  guard_scan_host(flat.data(), n, P.probes.data(), (uint32_t)P.n_points, (uint32_t)P.probes.size(), words.data());
  CHECK(words.back() == 0xDEADBEEFDEADBEEFull, "%s: the scan wrote past its words", what.c_str());
  if (n % 64) CHECK((words[guard_scan_words(n) - 1] >> (n % 64)) == 0, "%s: bits beyond the last plane are set", what.c_str());
  std::vector<size_t> counts;
  uint64_t first = 0;
  for (const MeshGuard &g : F.guards) {
    const std::vector<uint32_t> want = yardstick::risky_triangles(g, origins, F.lights);
    const std::vector<uint32_t> got = guard_scan_cut(words.data(), first, (uint32_t)(g.planes.size() / CTR_PLANE_DOUBLES));
    CHECK(got == want, "%s: mesh at plane %llu: %zu risky by the shared text, %zu by the old loop", what.c_str(), (unsigned long long)first, got.size(), want.size());
    counts.push_back(want.size());
    first += g.planes.size() / CTR_PLANE_DOUBLES;
  }
  // and the two plans: from the words, and from the host scan
  const GuardPlan from_words = plan_guards(F, P, words.data()), on_host = plan_guards(F, P, nullptr);
  CHECK(from_words.meshes.size() == on_host.meshes.size() && from_words.merged_keys == on_host.merged_keys && from_words.any_linear == on_host.any_linear, "%s: plans", what.c_str());
  for (size_t i = 0; i < on_host.meshes.size() && i < from_words.meshes.size(); i++) {
    CHECK(from_words.meshes[i].risky == on_host.meshes[i].risky && from_words.meshes[i].linear == on_host.meshes[i].linear, "%s: plan of mesh %zu", what.c_str(), i);
    CHECK(on_host.meshes[i].linear == (counts[i] > CTR_GUARD_SLOTS), "%s: mesh %zu: linear with %zu risky", what.c_str(), i, counts[i]);
  }
  return counts;
}

// leaf position `pos` of mesh `gi` gets the plane z = 0.5 (as guard_plane writes a plane: unit normal, a point, an extent)
static void put_in_plane(FlatScene &F, size_t gi, size_t pos, bool zero_area = false) {
  double *q = &F.guards[gi].planes[CTR_PLANE_DOUBLES * pos];
  q[0] = 0.0; q[1] = 0.0; q[2] = zero_area ? 0.0 : 1.0;
  q[3] = U(-1, 1); q[4] = U(-1, 1); q[5] = 0.5;
  q[6] = 0.3;
}

static void check_scan() {
  auto scene = [](const std::vector<size_t> &sizes, const std::vector<ctr_light> &lights) {
    Scene s;
    s.materials = {material(0.f, 0.f, 40.f)};
    s.lights = lights;
    for (size_t n : sizes) s.mesh(guard_tris(0, n, false), 0);
    s.cam.pos = ctr_vec3{0.3f, 0.8f, 4.03f};
    s.cam.w = s.cam.h = 16;
    s.finish();
    return s;
  };
  const std::vector<ctr_light> point = {light(CTR_LIGHT_POINT, 3.f, -1.f, 0.5f)}, sun = {light(CTR_LIGHT_SUN, 0.3f, -0.8f, 0.f)},
                               off = {light(CTR_LIGHT_POINT, 3.f, -1.f, 1.f), light(CTR_LIGHT_SUN, 0.3f, -0.8f, 0.5f), light(CTR_LIGHT_SUN, 0.f, 0.f, 0.f)};
  struct Probe { const char *what; std::vector<ctr_light> lights; bool eye_in_plane; };
  const Probe probes[] = {{"a point light", point, false}, {"a sun", sun, false}, {"no light, the eye", {}, true}, {"lights off the plane", off, false}};
  for (const Probe &pr : probes) {
    for (size_t n : {1u, 63u, 64u, 65u, 257u}) {
      for (size_t pos : {(size_t)0, (size_t)63, (size_t)64, n - 1}) {
        if (pos >= n) continue;
        Scene s = scene({n}, pr.lights);
        if (pr.eye_in_plane) { s.cam.pos.z = 0.5f; s.finish(); }
        FlatScene F = flat_of(s.desc);
        put_in_plane(F, 0, pos);
        if (n > 2) put_in_plane(F, 0, pos ? pos - 1 : 1, true);  // a zero-area neighbour in the plane: skipped
        const std::vector<size_t> c = scan_both(std::string(pr.what) + ", " + std::to_string(n) + " planes, position " + std::to_string(pos), F, cams_of(s.desc));
        const bool in_plane = strcmp(pr.what, "lights off the plane") != 0;
        CHECK(c[0] == (in_plane ? 1u : 0u), "%s, %zu planes, position %zu: %zu risky", pr.what, n, pos, c[0]);
        if (in_plane) {
          const GuardProbes P = guard_probes(F, cams_of(s.desc));
          CHECK(plan_guards(F, P, nullptr).meshes[0].risky == std::vector<uint32_t>(1, (uint32_t)pos), "%s: not position %zu", pr.what, pos);
        }
      }
    }
    // two meshes, 65 and 64: the last of the first, the first of the second
    Scene s = scene({65, 64}, pr.lights);
    if (pr.eye_in_plane) { s.cam.pos.z = 0.5f; s.finish(); }
    FlatScene F = flat_of(s.desc);
    put_in_plane(F, 0, 64);
    put_in_plane(F, 1, 0);
    std::vector<size_t> c = scan_both(std::string(pr.what) + ", meshes of 65 and 64", F, cams_of(s.desc));
    const bool in_plane = strcmp(pr.what, "lights off the plane") != 0;
    CHECK(c[0] == (in_plane ? 1u : 0u) && c[1] == c[0], "%s, meshes of 65 and 64: %zu and %zu risky", pr.what, c[0], c[1]);
    // 64 stay guarded, 65 go linear (scan_both checks `linear` against the count)
    for (size_t k : {64u, 65u}) {
      Scene t = scene({257}, pr.lights);
      if (pr.eye_in_plane) { t.cam.pos.z = 0.5f; t.finish(); }
      FlatScene G = flat_of(t.desc);
      for (size_t p = 0; p < k; p++) put_in_plane(G, 0, 3 * p + 1);
      c = scan_both(std::string(pr.what) + ", " + std::to_string(k) + " in the plane", G, cams_of(t.desc));
      CHECK(c[0] == (in_plane ? k : 0u), "%s: %zu in the plane, %zu risky", pr.what, k, c[0]);
    }
    printf("scan %-22s the shared text equals the old loop\n", pr.what);
  }
  // random planes against random probes, near and far from the tolerance
  for (int round = 0; round < 20; round++) {
    std::vector<ctr_light> lights;
    for (int k = 0; k < round % 5; k++) lights.push_back(light(k % 2 ? CTR_LIGHT_SUN : CTR_LIGHT_POINT, U(-2, 2), U(-2, 2), U(-2, 2)));
    Scene s = scene({(size_t)(1 + round * 13), 70}, lights);
    FlatScene F = flat_of(s.desc);
    for (MeshGuard &g : F.guards)
      for (size_t t = 0; t < g.planes.size() / CTR_PLANE_DOUBLES; t += 3) {  // every third plane through the eye, tilted by up to 4 tolerances
        double *q = &g.planes[CTR_PLANE_DOUBLES * t];
        const double tilt = U(-4.f, 4.f) / 131072.0;
        q[0] = tilt; q[1] = 0.0; q[2] = sqrt(1.0 - tilt * tilt);
        q[3] = 0.3 + U(-1, 1); q[4] = 0.8f; q[5] = 4.03f;
      }
    scan_both("random round " + std::to_string(round), F, cams_of(s.desc));
  }
  printf("scan random planes          the shared text equals the old loop\n");
}

int main(int argc, char **argv) {
  check_edits(argc, argv);
  check_scan();
  printf(fails ? "scene_edit_check: %d FAILURES\n" : "scene_edit_check: all checks hold\n", fails);
  return fails ? 1 : 0;
}
