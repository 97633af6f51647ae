// flatten_check.cpp — the host half of ctr_scene_create without a device: flatten_scene (cutrace_amd/csrc/scene_flatten.cpp) and
// the guard of the BVH culling (guard.cpp) on a scene description read from a file, everything they produce written to a dump
// that tests/test_scene_flatten.py checks.  No HIP; meant to run under ASan/UBSan as well.
//
//   flatten_check <scene.bin> <out.dump> [merge]
//
// scene.bin: uint64 n_objects, n_triangles, n_lights, n_materials, n_camera_sets; the ctr_object, ctr_triangle, ctr_light and
//            ctr_material arrays; the description's ctr_camera; per camera set a uint64 count and its ctr_camera array.
// out.dump : sections "<name> <bytes>\n<raw bytes>\n" — the flattened scene, then per camera set the plan, the dirty ranges and
//            the arrays after apply_guards; every set is planned TWICE, the second time must change nothing ("again").
//            `merge`: the merged tree is built after the first set and the set applied once more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "guard.h"
#include "scene_flatten.h"

static FILE *out;
static void section(const char *name, const void *p, size_t bytes) {
  fprintf(out, "%s %zu\n", name, bytes);
  if (bytes) fwrite(p, 1, bytes, out);
  fputc('\n', out);
}
template <class T> static void section(const char *name, const std::vector<T> &v) { section(name, v.data(), v.size() * sizeof(T)); }

template <class T> static std::vector<T> read_array(FILE *f, uint64_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "flatten_check: short scene file\n"); exit(3); }
  return v;
}

static void dump_arrays(const FlatScene &F) {
  section("objs", F.objs); section("oloop", F.oloop); section("meshes", F.meshes); section("planes", F.planes);
  section("tris", F.tris); section("nodes", F.nodes); section("nodes4", F.nodes4); section("gn", F.gn);
  section("lights", F.lights); section("mats", F.mats);
}

static void refresh(FlatScene &F, const std::vector<DCam> &cams, const char *what) {
  const GuardPlan plan = plan_guards(F, cams);
  const std::vector<DirtyRange> dirty = apply_guards(F, plan);
  section(what, nullptr, 0);
  const uint64_t p[5] = {plan.n_origins, plan.n_mirrors, plan.merged_keys.size(), plan.any_linear, plan.merged_usable()};
  section("plan", p, sizeof(p));
  std::vector<uint64_t> d;
  for (const DirtyRange &r : dirty) d.insert(d.end(), {(uint64_t)r.array, r.begin, r.count, r.payload.size()});
  section("dirty", d);
  for (const MeshGuard &g : F.guards) {
    section("guarded", g.guarded);
    const uint32_t lin = g.linear;
    section("linear", &lin, sizeof(lin));
  }
  const uint32_t m[2] = {F.merged.built, F.merged.usable};
  section("merged", m, sizeof(m));
  section("merged_guarded", F.merged.guarded);
  dump_arrays(F);
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: flatten_check <scene.bin> <out.dump> [merge]\n"); return 3; }
  const bool merge = argc > 3 && !strcmp(argv[3], "merge");
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 3; }
  const std::vector<uint64_t> n = read_array<uint64_t>(f, 5);
  const auto objects = read_array<ctr_object>(f, n[0]);
  const auto triangles = read_array<ctr_triangle>(f, n[1]);
  const auto lights = read_array<ctr_light>(f, n[2]);
  const auto materials = read_array<ctr_material>(f, n[3]);
  ctr_scene_desc d{objects.data(), n[0], triangles.data(), n[1], lights.data(), n[2], materials.data(), n[3], read_array<ctr_camera>(f, 1)[0]};
  std::vector<std::vector<DCam>> sets(n[4]);
  for (auto &set : sets)
    for (const ctr_camera &c : read_array<ctr_camera>(f, read_array<uint64_t>(f, 1)[0])) {
      DCam cam{};
      cam.pos[0] = c.pos.x; cam.pos[1] = c.pos.y; cam.pos[2] = c.pos.z;
      set.push_back(cam);
    }
  fclose(f);

  std::string err;
  if (validate_desc(d, err)) { printf("invalid: %s\n", err.c_str()); return 2; }
  FlatScene F;
  if (flatten_scene(d, F, err)) { printf("invalid: %s\n", err.c_str()); return 2; }
  out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 3; }
  dump_arrays(F);
  const uint64_t sc[17] = {F.n_mesh, F.tlas_root, F.tlas_begin, F.n_axis_recs, F.has_mesh, F.all_opaque, F.need_cold, F.any_bounce, F.mesh_tris,
                           F.mesh_bytes, F.ray_slots, F.merged.reserved, F.merged.tri_begin, F.merged.tri_count, F.merged.node_begin, F.merged.node_cap, F.fast_pow_ok};
  section("scalars", sc, sizeof(sc));
  std::vector<uint32_t> g;
  for (const MeshGuard &m : F.guards) g.insert(g.end(), {m.node_begin, m.node_count, m.tri_begin, m.tri_count, m.obj_index, (uint32_t)m.mesh_pos});
  section("guards", g);
  for (size_t k = 0; k < sets.size(); k++) {
    refresh(F, sets[k], "refresh");
    refresh(F, sets[k], "again");
    if (merge && k == 0) {
      std::vector<uint64_t> built;
      for (const DirtyRange &r : build_merged_tree(F)) built.insert(built.end(), {(uint64_t)r.array, r.begin, r.count, r.payload.size()});
      section("merged_built", built);
      refresh(F, sets[k], "refresh");
      refresh(F, sets[k], "again");
    }
  }
  fclose(out);
  printf("ok\n");
  return 0;
}
