// edit_check_common.h — what the edit check programs (scene_edit_check.cpp, object_edit_check.cpp, mesh_update_check.cpp,
// mesh_rebuild_check.cpp, mesh_replace_check.cpp, topology_check.cpp) share: a description that owns its arrays, the triangle sets, flatten + guard, the ONE restatement of
// ctr_scene_update_mesh on the host copy (update_on_host), and the byte-for-byte comparison of two flat scenes.
#ifndef CUTRACE_AMD_EDIT_CHECK_COMMON_H
#define CUTRACE_AMD_EDIT_CHECK_COMMON_H

#include <algorithm>
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
#include "mesh_refit.h"
#include "scene_flatten.h"
#include "tri_record.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 40) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::mt19937 rng(23);  // (mesh_update_check.cpp: rng.seed(11) before its first draw)
static float U(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

typedef std::vector<ctr_triangle> Tris;

// ---- a description that owns its arrays ----
struct Scene {
  std::vector<ctr_object> objects;
  Tris triangles;
  std::vector<ctr_light> lights;
  std::vector<ctr_material> materials;
  ctr_camera cam{};
  ctr_scene_desc desc{};
  void mesh(const Tris &t, uint64_t mat) {
    ctr_object o{};
    o.type = CTR_OBJ_MESH;
    o.mat_idx = mat;
    o.tri_begin = triangles.size();
    o.tri_count = t.size();
    ctr_mesh_bounds(t.data(), t.size(), &o.v0, &o.v1);
    triangles.insert(triangles.end(), t.begin(), t.end());
    objects.push_back(o);
  }
  void plane(ctr_vec3 p, ctr_vec3 n, uint64_t mat) {
    ctr_object o{};
    o.type = CTR_OBJ_PLANE;
    o.mat_idx = mat;
    o.v0 = p;
    o.v1 = n;
    objects.push_back(o);
  }
  void sphere(ctr_vec3 c, float r, uint64_t mat) {
    ctr_object o{};
    o.type = CTR_OBJ_SPHERE;
    o.mat_idx = mat;
    o.v0 = c;
    o.f0 = r;
    objects.push_back(o);
  }
  void triangle(ctr_vec3 p1, ctr_vec3 p2, ctr_vec3 p3, uint64_t mat) {
    ctr_object o{};
    o.type = CTR_OBJ_TRIANGLE;
    o.mat_idx = mat;
    o.v0 = p1;
    o.v1 = p2;
    o.v2 = p3;
    objects.push_back(o);
  }
  const ctr_scene_desc &finish() {
    desc.objects = objects.data(); desc.n_objects = objects.size();
    desc.triangles = triangles.data(); desc.n_triangles = triangles.size();
    desc.lights = lights.data(); desc.n_lights = lights.size();
    desc.materials = materials.data(); desc.n_materials = materials.size();
    desc.cam = cam;
    return desc;
  }
  static Scene copy_of(const ctr_scene_desc &d) {
    Scene s;
    s.objects.assign(d.objects, d.objects + d.n_objects);
    s.triangles.assign(d.triangles, d.triangles + d.n_triangles);
    s.lights.assign(d.lights, d.lights + d.n_lights);
    s.materials.assign(d.materials, d.materials + d.n_materials);
    s.cam = d.cam;
    s.finish();
    return s;
  }
};

static ctr_light light(uint32_t type, float x, float y, float z, float c = 0.8f) {
  ctr_light l{};
  l.type = type;
  l.v = ctr_vec3{x, y, z};
  l.color = ctr_vec3{c, c, c};
  return l;
}

static ctr_material material(float reflect, float transparency, float phong) {
  ctr_material m{};
  m.type = CTR_MAT_PHONG;
  m.color = ctr_vec3{0.8f, 0.6f, 0.3f};
  m.specular = 0.4f;
  m.reflexivity = reflect;
  m.phong_exp = phong;
  m.transparency = transparency;
  return m;
}

// k triangles in the plane z = 0.5 (file indices 0 .. k-1), n_other in tilted planes that hold no probe used here, two of no area
static Tris guard_tris(size_t k, size_t n_other, bool zero_area = true) {
  Tris t;
  auto tri = [&](float zc, float slope) {
    const float x = U(-1, 1), y = U(-1, 1);
    auto z = [&](float px) { return zc + slope * px; };
    t.push_back(ctr_triangle{{x, y, z(x)}, {x + 0.3f, y + 0.05f, z(x + 0.3f)}, {x + 0.1f, y + 0.35f, z(x + 0.1f)}});
  };
  for (size_t i = 0; i < k; i++) tri(0.5f, 0.f);
  for (size_t j = 0; j < n_other; j++) tri(2.0f + 0.1f * (float)j, 0.2f);
  if (zero_area) {
    t.push_back(ctr_triangle{{0.1f, 0.1f, 0.5f}, {0.1f, 0.1f, 0.5f}, {0.1f, 0.1f, 0.5f}});
    t.push_back(ctr_triangle{{0, 0, 0.5f}, {0.5f, 0.5f, 0.5f}, {1, 1, 0.5f}});
  }
  return t;
}

static FlatScene flat_of(const ctr_scene_desc &d) {
  FlatScene F;
  std::string err;
  if (validate_desc(d, err) || flatten_scene(d, F, err)) { printf("FAIL flatten: %s\n", err.c_str()); exit(1); }
  return F;
}

static std::vector<DCam> cams_of(const ctr_scene_desc &d) {
  DCam c{};
  c.pos[0] = d.cam.pos.x; c.pos[1] = d.cam.pos.y; c.pos[2] = d.cam.pos.z;
  return std::vector<DCam>(1, c);
}

static void guard(FlatScene &F, const std::vector<DCam> &cams) { apply_guards(F, plan_guards(F, cams)); }

// ... with one camera at `eye`; returns what the device would have to receive
static std::vector<DirtyRange> guard(FlatScene &F, const float *eye) {
  DCam c{};
  for (int a = 0; a < 3; a++) c.pos[a] = eye[a];
  return apply_guards(F, plan_guards(F, std::vector<DCam>(1, c)));
}

// ---- triangle sets (every draw is one of `rng`: a program that reads its own lines seeds it before the first) ----
static Tris random_tris(size_t n, float spread, float size) {
  Tris t(n);
  for (ctr_triangle &q : t) {
    const ctr_vec3 o{U(-spread, spread), U(-spread, spread), U(-spread, spread)};
    ctr_vec3 *p[3] = {&q.p1, &q.p2, &q.p3};
    for (ctr_vec3 *v : p) *v = ctr_vec3{o.x + U(-size, size), o.y + U(-size, size), o.z + U(-size, size)};
  }
  return t;
}

// a rotation about (1, 2, 3) by `angle` plus a per-vertex wobble
static Tris moved(const Tris &t, float angle, float wobble) {
  const double k[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)}, c = std::cos(angle), s = std::sin(angle);
  auto rot = [&](ctr_vec3 v) {
    const double d = k[0] * v.x + k[1] * v.y + k[2] * v.z;
    const double cr[3] = {k[1] * v.z - k[2] * v.y, k[2] * v.x - k[0] * v.z, k[0] * v.y - k[1] * v.x};
    return ctr_vec3{(float)(v.x * c + cr[0] * s + k[0] * d * (1 - c)) + U(-wobble, wobble), (float)(v.y * c + cr[1] * s + k[1] * d * (1 - c)) + U(-wobble, wobble),
                    (float)(v.z * c + cr[2] * s + k[2] * d * (1 - c)) + U(-wobble, wobble)};
  };
  Tris out(t);
  for (ctr_triangle &q : out) { q.p1 = rot(q.p1); q.p2 = rot(q.p2); q.p3 = rot(q.p3); }
  return out;
}

// `k` of the mesh's triangles (file indices 0 .. k-1) in the plane z = 0.5, the others where they were
static Tris with_in_plane(const Tris &t, size_t k) {
  Tris out(t);
  for (size_t i = 0; i < k && i < out.size(); i++) {
    const float x = U(-1, 1), y = U(-1, 1);
    out[i].p1 = ctr_vec3{x, y, 0.5f}; out[i].p2 = ctr_vec3{x + 0.3f, y + 0.05f, 0.5f}; out[i].p3 = ctr_vec3{x + 0.1f, y + 0.35f, 0.5f};
  }
  return out;
}

// ---- the device's half of an update, restated ----
// the refit of one tree on the host, level by level as the device launches it
static void refit_on_host(DNode4 *nodes, const LevelSchedule &S, const DTri *recs, const Tris &verts) {
  for (size_t h = 0; h < S.levels(); h++)
    for (uint32_t i = S.begin[h]; i < S.begin[h + 1]; i++)
      for (int c = 0; c < 4; c++) refit_slot(nodes, S.nodes[i], c, recs, &verts[0].p1.x);
}

// min / max over the vertices of every triangle below descriptor `d`
static void brute(const std::vector<DNode4> &nodes, uint32_t d, const std::vector<uint32_t> &order, const Tris &verts, float *lo, float *hi) {
  if (d == BVH_LEAF_FLAG) return;
  if (d & BVH_LEAF_FLAG) {
    for (uint32_t k = d & 0xFFFFFFu; k < (d & 0xFFFFFFu) + ((d >> 24) & 0x7Fu); k++) {
      const float *v = &verts[order[k]].p1.x;
      for (int j = 0; j < 9; j++) { lo[j % 3] = std::min(lo[j % 3], v[j]); hi[j % 3] = std::max(hi[j % 3], v[j]); }
    }
    return;
  }
  for (int c = 0; c < 4; c++) brute(nodes, nodes[d].child[c], order, verts, lo, hi);
}

// ctr_scene_update_mesh on the host copy: what update_tris, refit_level and mesh_box do on the device, then mesh_updated
static void update_on_host(FlatScene &F, size_t gi, const Tris &nt) {
  MeshGuard &g = F.guards[gi];
  for (uint32_t k = 0; k < g.tri_count; k++) {
    const uint32_t orig = F.tris[g.tri_begin + k].orig;
    make_tri(nt[orig].p1, nt[orig].p2, nt[orig].p3, orig, F.tris[g.tri_begin + k], &F.gn[4 * (g.tri_begin + orig)]);
    guard_plane(nt[orig].p1, nt[orig].p2, nt[orig].p3, &g.planes[CTR_PLANE_DOUBLES * k]);
  }
  LevelSchedule S;
  CHECK(level_schedule(&F.nodes4[g.node_begin], g.node_count, g.tri_count, S), "update: no schedule");
  refit_on_host(&F.nodes4[g.node_begin], S, &F.tris[g.tri_begin], nt);
  float box[6];
  refit_mesh_box(F.nodes4[g.node_begin], box);
  mesh_updated(F, gi, box);
}

template <class T> static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// A (edited in place) against B (flattened from the edited description), both guarded
static void same_flat(const std::string &what, const FlatScene &A, const FlatScene &B) {
  const char *w = what.c_str();
  CHECK(same_bytes(A.objs, B.objs), "%s: objs", w);
  CHECK(same_bytes(A.oloop, B.oloop), "%s: oloop", w);
  // a merged tree that mesh_updated retired (room in the arrays, reserved no more) is never walked again: where its walk would
  // start, its guard records and its spare nodes are whatever its last state left
  const bool retired = !A.merged.reserved && !B.merged.reserved && A.merged.tri_count != 0 && B.merged.tri_count != 0;
  std::vector<DObj> ma = A.meshes, mb = B.meshes;
  if (retired && ma.size() > A.n_mesh && mb.size() > A.n_mesh) ma[A.n_mesh].bvh_root = mb[A.n_mesh].bvh_root = 0;
  CHECK(same_bytes(ma, mb), "%s: meshes", w);
  CHECK(same_bytes(A.planes, B.planes), "%s: planes", w);
  CHECK(same_bytes(A.nodes, B.nodes), "%s: nodes", w);
  CHECK(same_bytes(A.lights, B.lights), "%s: lights", w);
  CHECK(same_bytes(A.mats, B.mats), "%s: mats", w);
  CHECK(A.all_opaque == B.all_opaque && A.need_cold == B.need_cold && A.any_bounce == B.any_bounce && A.fast_pow_ok == B.fast_pow_ok,
        "%s: flags %d%d%d%d / %d%d%d%d", w, A.all_opaque, A.need_cold, A.any_bounce, A.fast_pow_ok, B.all_opaque, B.need_cold, B.any_bounce, B.fast_pow_ok);
  CHECK(A.n_mesh == B.n_mesh && A.tlas_root == B.tlas_root && A.tlas_begin == B.tlas_begin && A.n_axis_recs == B.n_axis_recs && A.has_mesh == B.has_mesh &&
        A.mesh_tris == B.mesh_tris && A.mesh_bytes == B.mesh_bytes && A.ray_slots == B.ray_slots && !memcmp(A.tl_mn, B.tl_mn, 12) && !memcmp(A.tl_mx, B.tl_mx, 12),
        "%s: scalars", w);
  // tris, gn, nodes4: all but the records nothing reads (beyond the current guard state)
  CHECK(A.tris.size() == B.tris.size() && A.gn.size() == B.gn.size() && A.nodes4.size() == B.nodes4.size() && A.guards.size() == B.guards.size(), "%s: sizes", w);
  if (A.tris.size() != B.tris.size() || A.nodes4.size() != B.nodes4.size() || A.guards.size() != B.guards.size()) return;
  std::vector<uint8_t> skip_tri(A.tris.size(), 0), skip_node(A.nodes4.size(), 0);
  for (size_t i = 0; i < A.guards.size(); i++) {
    const MeshGuard &ga = A.guards[i], &gb = B.guards[i];
    CHECK(ga.guarded == gb.guarded && ga.linear == gb.linear, "%s: mesh %zu: guarded %zu / %zu, linear %d / %d", w, i, ga.guarded.size(), gb.guarded.size(), (int)ga.linear, (int)gb.linear);
    CHECK(same_bytes(ga.planes, gb.planes) && ga.node_begin == gb.node_begin && ga.node_count == gb.node_count && ga.tri_begin == gb.tri_begin &&
          ga.tri_count == gb.tri_count && ga.obj_index == gb.obj_index && ga.mesh_pos == gb.mesh_pos, "%s: mesh %zu: guard record", w, i);
    if (ga.mesh_pos < 0) continue;
    for (uint32_t k = (uint32_t)ga.guarded.size(); k < CTR_GUARD_SLOTS; k++) skip_tri[ga.tri_begin + ga.tri_count + k] = 1;
    if (ga.guarded.empty()) skip_node[ga.node_begin + ga.node_count] = 1;
  }
  CHECK(A.merged.reserved == B.merged.reserved && A.merged.built == B.merged.built && A.merged.usable == B.merged.usable &&
        (!A.merged.usable || A.merged.guarded == B.merged.guarded) && A.merged.where == B.merged.where, "%s: merged tree: usable %d / %d, keys %zu / %zu", w,
        (int)A.merged.usable, (int)B.merged.usable, A.merged.guarded.size(), B.merged.guarded.size());
  if (A.merged.built || retired) {
    const Merged &M = A.merged;
    // (a tree that is not usable is not walked: its keys and guard records are whatever the last usable state left)
    for (size_t k = M.usable ? M.guarded.size() : 0; k < CTR_GUARD_SLOTS; k++) skip_tri[M.tri_begin + M.tri_count + k] = 1;
    size_t groups = 0;
    for (size_t k = 0; M.usable && k < M.guarded.size(); k++) groups += k == 0 || (M.guarded[k] >> 24) != (M.guarded[k - 1] >> 24);
    for (size_t j = (groups + 2) / 3; j < CTR_MERGED_SPARE_NODES; j++) skip_node[M.node_begin + M.node_count + j] = 1;
  }
  size_t bad = 0;
  for (size_t k = 0; k < A.tris.size(); k++)
    if (!skip_tri[k]) bad += memcmp(&A.tris[k], &B.tris[k], sizeof(DTri)) != 0 || memcmp(&A.gn[4 * k], &B.gn[4 * k], 16) != 0;
  CHECK(bad == 0, "%s: %zu triangle records or normals differ", w, bad);
  bad = 0;
  for (size_t k = 0; k < A.nodes4.size(); k++)
    if (!skip_node[k]) bad += memcmp(&A.nodes4[k], &B.nodes4[k], sizeof(DNode4)) != 0;
  CHECK(bad == 0, "%s: %zu mesh nodes differ", w, bad);
}

#endif
