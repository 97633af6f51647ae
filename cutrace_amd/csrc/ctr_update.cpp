// ctr_update.cpp — the host half of include/cutrace_update.h (ctr_scene_update_mesh, ctr_scene_mesh_box), of
// include/cutrace_rebuild.h (ctr_scene_rebuild_mesh) and of include/cutrace_replace.h (ctr_scene_replace_mesh).  No HIP kernels
// here: the device halves are mesh_update.hip and mesh_build.hip, the arithmetic both sides share is tri_record.h, mesh_refit.h
// and lbvh.h.
//
// An update in five steps:
//   1. arguments and vertices are checked; nothing of the handle has changed when the call fails here
//   2. the device rebuilds the mesh's DTri records, normals and guard planes from the new vertices and refits its tree,
//      level by level (the level schedule: mesh_refit.h, derived at the mesh's first update and kept on the handle)
//   3. what the device wrote comes back into the host copy, through a page-locked buffer, in one wait.  FlatScene stays the
//      authority: the guard, the mirrors, the scene head and the payload of a linear mesh all read it
//   4. mesh_updated (scene_flatten.cpp) derives the rest on the host: the mesh's box in its records, the top-level tree, the
//      guard state reset, the merged tree retired
//   5. upload_dirty and refresh_linear_meshes, the machinery ctr_scene_set_cameras ends with; the guard's plane scan runs on the
//      device when it is large enough (guard_scan.h), over the planes step 2 left there
//
// A rebuild is an update with three steps between 1 and 2:
//   1a. a tree SHAPE over the new vertices: the device's linear BVH (mesh_build.hip, into scratch buffers of the handle, its
//       descriptors and sorted indices copied back) or the host's bvh4_build
//   1b. the host accepts the device's tree (lbvh.h lbvh_accept) or builds one itself; the new level schedule, the room the
//       tree needs in the device's node array and every buffer of steps 2 .. 5 are allocated.  Still nothing has changed
//   1c. mesh_rebuilt (scene_flatten.cpp) installs the shape in the host copy; the device receives the descriptors and the
//       records' new `orig`
// and steps 2 .. 5 run with the NEW schedule.
//
// A replace is a rebuild whose triangle count may differ from the mesh's: 1b also works out where the mesh's triangle and node
// ranges will live (scene_flatten.h replace_room) and grows d_tris, d_gnorm and d_nodes4 for them, and 1c is mesh_replaced.
//
// An add (ctr_scene_add_mesh, include/cutrace_topology.h; the other calls of that header are ctr_topology.cpp) is a replace of a mesh
// that is not there yet: 1 checks a material index where the others look for the mesh, 1b asks add_room, which knows the ranges that
// removed objects left behind, and also gives d_objs, d_meshes and d_nodes room for one mesh more, 1c is mesh_added, and step 4 is
// mesh_joined: the top-level tree can be built only once the device has said what the mesh's box is.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "ctr_internal.h"
#include "cutrace_rebuild.h"
#include "cutrace_replace.h"
#include "cutrace_topology.h"
#include "cutrace_update.h"
#include "guard.h"
#include "mesh_build.h"
#include "mesh_refit.h"
#include "mesh_update.h"

namespace {

enum class Where { HOST, DEVICE, ELSEWHERE };

// where `bytes` bytes at `p` live, as far as ctr_scene_update_mesh cares: host memory (page-locked or not), memory of
// `device` (the test of check_device_pointers, at the first and the last byte), or anything else
Where where_is(const void *p, size_t bytes, int device) {
  auto one = [&](const void *q) {
    const MemKind m = memory_kind(q);
    if (m.kind == MemKind::DEVICE) return m.device == device ? Where::DEVICE : Where::ELSEWHERE;
    return m.kind == MemKind::ELSEWHERE ? Where::ELSEWHERE : Where::HOST;
  };
  const Where first = one(p), last = one((const char *)p + bytes - 1);
  return first == last ? first : Where::ELSEWHERE;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// the level schedule of a tree, on the host and on the device
int refit_of_tree(const DNode4 *nodes, uint32_t node_count, uint32_t tri_count, const std::string &who, std::unique_ptr<MeshRefit> &out) {
  auto r = std::make_unique<MeshRefit>();
  if (!level_schedule(nodes, node_count, tri_count, r->sched)) return fail(CTR_E_INVALID, who + "the mesh's tree is not one the refit can walk");
  if (int st = r->d_nodes.reserve(r->sched.nodes.size())) return st;
  HIP_TRY(hipMemcpy(r->d_nodes.p, r->sched.nodes.data(), r->sched.nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  out = std::move(r);
  return CTR_OK;
}

// the mesh's level schedule from the host copy of its tree: once per mesh and tree
int mesh_refit_of(ctr_scene *s, size_t gi, MeshRefit **out) {
  if (s->refit.size() < s->flat.guards.size()) s->refit.resize(s->flat.guards.size());
  if (!s->refit[gi]) {
    const FlatScene &F = s->flat;
    const MeshGuard &g = F.guards[gi];
    // (the kernels index the caller's vertices by a record's `orig`: it must name a triangle of the mesh)
    bool ok = true;
    for (uint32_t k = 0; ok && k < g.tri_count; k++) ok = F.tris[g.tri_begin + k].orig < g.tri_count;
    if (!ok) return fail(CTR_E_INVALID, "ctr_scene_update_mesh: the mesh's tree is not one the refit can walk");
    if (int st = refit_of_tree(&F.nodes4[g.node_begin], g.node_count, g.tri_count, "ctr_scene_update_mesh: ", s->refit[gi])) return st;
  }
  *out = s->refit[gi].get();
  return CTR_OK;
}

// CUTRACE_DEBUG_UPDATE=1: where ctr_scene_update_mesh and ctr_scene_rebuild_mesh spend their time (stderr), the time since the
// previous stamp; the device kernels then get a wait of their own, so that their time is not counted as the copy-back's
// (scripts/gpu_mesh_update.py, scripts/gpu_mesh_rebuild.py)
struct Stamps {
  const char *call;
  const bool on = getenv("CUTRACE_DEBUG_UPDATE") != nullptr;
  std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
  explicit Stamps(const char *call_name) : call(call_name) {}
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::high_resolution_clock::now();
    fprintf(stderr, "cutrace_amd %s: %-24s %8.3f ms\n", call, what, std::chrono::duration<double, std::milli>(now - t0).count());
    t0 = now;
  }
};

// where the parts of the copy-back land in ctr_scene::upd_back, for a mesh of `n` triangles and `node_count` nodes
struct BackLayout {
  size_t tris, gn, nodes, planes, box, flag, end;
  BackLayout(uint32_t n, uint32_t node_count) {
    tris = 0;
    gn = tris + align16(n * sizeof(DTri));
    nodes = gn + align16(n * 4 * sizeof(float));
    planes = nodes + align16(node_count * sizeof(DNode4));
    box = planes + align16(n * CTR_PLANE_DOUBLES * sizeof(double));
    flag = box + 32;
    end = flag + 16;
  }
};

// What the three calls share: the edit they are (the handle's lock from here on), and what is known once the arguments name a mesh
struct MeshCall {
  const Edit edit;
  ctr_scene *s;
  std::string who;
  size_t gi = 0;
  uint32_t n = 0;
  const ctr_triangle *tris = nullptr;
  Where where = Where::HOST;
  hipStream_t stream = nullptr;
  const float *d_verts = nullptr;  // the vertices on the device: the caller's, or upd_verts once upload_verts has run
  bool uploaded = false;
  bool adding = false;             // ctr_scene_add_mesh: the mesh is the last of the list once mesh_added has run
  uint64_t mat_idx = 0;            // ... and this its material
  Stamps stamp;
  MeshCall(ctr_scene *scene, const char *name) : edit(scene), s(scene), who(std::string(name) + ": "), stamp(name + 10 /* past "ctr_scene_" */) {}
};

// ---- 1. the arguments: `object` is a non-empty mesh of n_tris triangles — or, with any_count, of any number of them and n_tris a
// count a mesh may have; the scene's device becomes current ----
int mesh_arguments(MeshCall &c, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, void *hip_stream, bool any_count = false) {
  const FlatScene &F = c.s->flat;
  if (object >= F.objs.size() || F.objs[object].type != CTR_OBJ_MESH)
    return fail(CTR_E_INVALID, c.who + "object #" + std::to_string(object) + " is not a mesh");
  if (F.objs[object].tri_count == 0) return fail(CTR_E_INVALID, c.who + "object #" + std::to_string(object) + " is an empty mesh");
  if (any_count && (n_tris == 0 || n_tris > CTR_MESH_TRIS_MAX))
    return fail(CTR_E_INVALID, c.who + std::to_string(n_tris) + " triangles: a mesh has 1 .. " + std::to_string(CTR_MESH_TRIS_MAX));
  if (!any_count && n_tris != F.objs[object].tri_count)
    return fail(CTR_E_INVALID, c.who + std::to_string(n_tris) + " triangles for a mesh of " + std::to_string(F.objs[object].tri_count) +
                                   ": the count is fixed");
  size_t gi = 0;
  while (gi < F.guards.size() && F.guards[gi].obj_index != object) gi++;
  if (gi == F.guards.size() || F.guards[gi].mesh_pos < 0) return fail(CTR_E_INVALID, c.who + "the mesh has no records");
  c.gi = gi;
  c.n = (uint32_t)n_tris;
  c.tris = tris;
  c.stream = (hipStream_t)hip_stream;
  if (int st = use_device(c.s)) return st;
  c.where = where_is(tris, c.n * sizeof(ctr_triangle), c.s->device);
  if (c.where == Where::ELSEWHERE) return fail(CTR_E_INVALID, c.who + "tris is neither host memory nor device memory of the scene's device");
  return CTR_OK;
}

// ---- 1. of an add: a material of the scene and a count a mesh may have; the scene's device becomes current ----
int add_arguments(MeshCall &c, uint64_t mat_idx, const ctr_triangle *tris, uint64_t n_tris, void *hip_stream) {
  const FlatScene &F = c.s->flat;
  if (mat_idx >= F.mats.size()) return fail(CTR_E_INVALID, c.who + "material index " + std::to_string(mat_idx) + " out of range");
  if (n_tris == 0 || n_tris > CTR_MESH_TRIS_MAX)
    return fail(CTR_E_INVALID, c.who + std::to_string(n_tris) + " triangles: a mesh has 1 .. " + std::to_string(CTR_MESH_TRIS_MAX));
  if (F.objs.size() >= 0xFFFFFFFFull) return fail(CTR_E_INVALID, c.who + "scene too large for 32-bit device indices");
  c.adding = true;
  c.mat_idx = mat_idx;
  c.n = (uint32_t)n_tris;
  c.tris = tris;
  c.stream = (hipStream_t)hip_stream;
  if (int st = use_device(c.s)) return st;
  c.where = where_is(tris, c.n * sizeof(ctr_triangle), c.s->device);
  if (c.where == Where::ELSEWHERE) return fail(CTR_E_INVALID, c.who + "tris is neither host memory nor device memory of the scene's device");
  return CTR_OK;
}

// ---- 1. the vertices must be finite; the buffers of steps 2 and 3 for a tree of up to `node_count` nodes (nothing of the scene changes) ----
int vertices_and_buffers(MeshCall &c, uint32_t node_count) {
  ctr_scene *s = c.s;
  const uint32_t n = c.n;
  const BackLayout b(n, node_count);
  if (int st = s->upd_back.reserve(b.end)) return st;
  if (int st = s->upd_planes.reserve(n)) return st;
  if (int st = s->upd_words.reserve(8)) return st;
  char *back = s->upd_back.as<char>();
  uint32_t *d_flag = s->upd_words.as<uint32_t>();
  c.d_verts = (const float *)c.tris;
  if (c.where == Where::HOST) {
    const float *v = (const float *)c.tris;
    for (size_t i = 0; i < 9 * (size_t)n; i++)
      if (!std::isfinite(v[i])) return fail(CTR_E_INVALID, c.who + "triangle " + std::to_string(i / 9) + " has a vertex that is not finite");
    if (int st = s->upd_verts.reserve(n)) return st;
    c.d_verts = s->upd_verts.as<float>();
  } else {
    // a small kernel of its own, its one flag word read back before anything is modified
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), c.stream));
    if (int st = launched(ctr_launch_all_finite(c.d_verts, 9 * (uint64_t)n, d_flag, c.stream), "finiteness check launch")) return st;
    HIP_TRY(hipMemcpyAsync(back + b.flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    uint32_t flag;
    memcpy(&flag, back + b.flag, sizeof(flag));
    if (flag) return fail(CTR_E_INVALID, c.who + "a vertex is not finite");
  }
  return CTR_OK;
}

// a host input's vertices go to the device, on the caller's stream (once per call; upd_verts is scratch, not scene)
int upload_verts(MeshCall &c) {
  if (c.where == Where::HOST && !c.uploaded)
    HIP_TRY(hipMemcpyAsync(c.s->upd_verts.p, c.tris, c.n * sizeof(ctr_triangle), hipMemcpyHostToDevice, c.stream));
  c.uploaded = true;
  return CTR_OK;
}

// ---- 2. .. 5.: the device side on the caller's stream, the copy-back, everything derived, the guard ----
int update_steps(MeshCall &c, const MeshRefit *refit) {
  ctr_scene *s = c.s;
  FlatScene &F = s->flat;
  const uint32_t n = c.n;
  const uint32_t tri_begin = F.guards[c.gi].tri_begin, node_begin = F.guards[c.gi].node_begin, node_count = F.guards[c.gi].node_count;
  const BackLayout b(n, node_count);
  char *back = s->upd_back.as<char>();
  float *d_box = s->upd_words.as<float>() + 2;
  const float *d_verts = c.d_verts;
  hipStream_t stream = c.stream;
  Stamps &stamp = c.stamp;
  if (int st = upload_verts(c)) return st;
  DTri *d_recs = s->d_tris.as<DTri>() + tri_begin;
  float *d_gn = s->d_gnorm.as<float>() + 4 * (size_t)tri_begin;
  DNode4 *d_nodes = s->d_nodes4.as<DNode4>() + node_begin;  // (the mesh's spare node and guard records are not the kernels' business)
  double *d_planes = s->upd_planes.as<double>();
  if (int st = launched(ctr_launch_update_tris(d_recs, d_gn, d_planes, d_verts, n, stream), "update_tris launch")) return st;
  const LevelSchedule &sched = refit->sched;
  for (size_t h = 0; h < sched.levels(); h++)
    if (int st = launched(ctr_launch_refit_level(d_nodes, refit->d_nodes.as<uint32_t>() + sched.begin[h], sched.begin[h + 1] - sched.begin[h],
                                                 d_recs, d_verts, stream), "refit_level launch"))
      return st;
  if (int st = launched(ctr_launch_mesh_box(d_nodes, d_box, stream), "mesh_box launch")) return st;

  if (stamp.on) HIP_TRY(hipStreamSynchronize(stream));
  stamp("upload + device kernels");

  // ---- 3. back into the host copy: one wait ----
  HIP_TRY(hipMemcpyAsync(back + b.tris, d_recs, n * sizeof(DTri), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b.gn, d_gn, n * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b.nodes, d_nodes, node_count * sizeof(DNode4), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b.planes, d_planes, n * CTR_PLANE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b.box, d_box, 6 * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  MeshGuard &g = F.guards[c.gi];
  memcpy(&F.tris[tri_begin], back + b.tris, n * sizeof(DTri));
  memcpy(&F.gn[4 * (size_t)tri_begin], back + b.gn, n * 4 * sizeof(float));
  memcpy(&F.nodes4[node_begin], back + b.nodes, node_count * sizeof(DNode4));
  memcpy(g.planes.data(), back + b.planes, n * CTR_PLANE_DOUBLES * sizeof(double));
  float box[6];
  memcpy(box, back + b.box, sizeof(box));
  stamp("copy-back");

  // ---- 4., 5. everything derived from them, then the guard ----
  const std::vector<DirtyRange> derived = c.adding ? mesh_joined(F, c.gi, box) : mesh_updated(F, c.gi, box);
  // (holds while a top-level tree over m meshes has fewer than m nodes; nothing is uploaded past the end of an array whatever the builder does)
  if (F.nodes.size() > s->d_nodes.cap || F.meshes.size() > s->d_meshes.cap) return fail(CTR_E_INVALID, c.who + "a larger top-level tree than its arrays have room for");
  if (int st = upload_dirty(s, derived)) return st;
  stamp("host records + upload");
  // (the new planes are on the device already, in upd_planes, and the stream has been waited for: the scan takes them from there)
  if (int st = guard_planes_changed(s, c.gi, d_planes)) return st;
  const int st = c.edit.end({}, true);  // (the records went up above, ahead of their stamp)
  stamp("guard");
  return st;
}

// ---- 1a. the device builder: a tree shape over c.d_verts into scratch, its descriptors and sorted indices back on the host ----
// sparse: max(n - 1, 1) descriptors indexed by binary node; order: n file indices.  Waits for the stream.
int device_shape(MeshCall &c, std::vector<DNode4> &sparse, std::vector<uint32_t> &order) {
  ctr_scene *s = c.s;
  const uint32_t n = c.n, n_sparse = n > 1 ? n - 1 : 1;
  size_t temp_bytes = 0;
  if (int st = launched(ctr_lbvh_sort_temp_bytes(n, &temp_bytes), "radix sort size query")) return st;
  if (int st = s->rb_keys.reserve(2 * (size_t)n)) return st;
  if (int st = s->rb_index.reserve(2 * (size_t)n)) return st;
  if (int st = s->rb_temp.reserve(temp_bytes ? temp_bytes : 16)) return st;
  if (int st = s->rb_bin.reserve(n_sparse)) return st;
  if (int st = s->rb_nodes.reserve(n_sparse)) return st;
  if (int st = s->rb_words.reserve(8 + ctr_lbvh_partial_floats(n))) return st;
  const size_t b_nodes = 0, b_order = align16(n_sparse * sizeof(DNode4)), b_end = b_order + align16(n * sizeof(uint32_t));
  if (int st = s->upd_back.reserve(b_end)) return st;
  hipStream_t stream = c.stream;
  uint64_t *keys = s->rb_keys.as<uint64_t>(), *keys_sorted = keys + n;
  uint32_t *index = s->rb_index.as<uint32_t>(), *index_sorted = index + n;
  float *bounds = s->rb_words.as<float>();
  if (int st = upload_verts(c)) return st;
  if (int st = launched(ctr_launch_lbvh_bounds(c.d_verts, n, bounds + 8, bounds, stream), "centroid bounds launch")) return st;
  if (int st = launched(ctr_launch_lbvh_keys(c.d_verts, n, bounds, keys, index, stream), "morton keys launch")) return st;
  if (int st = launched(ctr_lbvh_sort(s->rb_temp.p, temp_bytes, keys, keys_sorted, index, index_sorted, n, stream), "radix sort")) return st;
  if (c.stamp.on) HIP_TRY(hipStreamSynchronize(stream));
  c.stamp("sort");
  if (int st = launched(ctr_launch_lbvh_tree(keys_sorted, n, s->rb_bin.as<LbvhNode>(), stream), "radix tree launch")) return st;
  if (int st = launched(ctr_launch_lbvh_collapse(s->rb_bin.as<LbvhNode>(), keys_sorted, n, BVH_LEAF, s->rb_nodes.as<DNode4>(), stream), "collapse launch")) return st;
  if (c.stamp.on) HIP_TRY(hipStreamSynchronize(stream));
  c.stamp("tree + collapse");
  char *back = s->upd_back.as<char>();
  HIP_TRY(hipMemcpyAsync(back + b_nodes, s->rb_nodes.p, n_sparse * sizeof(DNode4), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b_order, index_sorted, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sparse.resize(n_sparse);
  order.resize(n);
  memcpy(sparse.data(), back + b_nodes, n_sparse * sizeof(DNode4));
  memcpy(order.data(), back + b_order, n * sizeof(uint32_t));
  c.stamp("shape copy-back");
  return CTR_OK;
}

// What a rebuild or a replace built and moved: the fields of ctr_rebuild_info and ctr_replace_info
// (of an add: the two `moved` say that the range is one a removed object left behind)
struct Built { uint32_t builder = 0, fell_back = 0, node_count = 0, levels = 0, nodes_moved = 0, tris_moved = 0, tri_cap = 0; };

// ---- a rebuild (the count is the mesh's), a replace (any count) or — the arguments checked already — an add: steps 1 .. 5 ----
int rebuild_or_replace(MeshCall &c, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, bool host_builder, bool replace, void *hip_stream,
                       Built &built) {
  ctr_scene *s = c.s;
  const std::string &who = c.who;
  if (!c.adding)
    if (int st = mesh_arguments(c, object, tris, n_tris, hip_stream, replace)) return st;
  FlatScene &F = s->flat;
  const uint32_t n = c.n;
  if (int st = vertices_and_buffers(c, n)) return st;  // (a four-wide tree over n triangles has at most n nodes)
  c.stamp("checks");

  // ---- 1a., 1b. a tree: the device's, accepted; or the host's ----
  MeshTree tree;
  if (!host_builder) {
    std::vector<DNode4> sparse;
    if (int st = device_shape(c, sparse, tree.order)) return st;
    if (!lbvh_accept(sparse.data(), (uint32_t)sparse.size(), tree.order.data(), n, BVH_LEAF, tree.nodes)) built.fell_back = 1;
    c.stamp("host accept");
  }
  if (host_builder || built.fell_back) {
    built.builder = 1;
    std::vector<ctr_triangle> from_device;
    const ctr_triangle *host_tris = tris;
    if (c.where == Where::DEVICE) {  // (the finiteness check has waited for whatever produced them)
      from_device.resize(n);
      HIP_TRY(hipMemcpy(from_device.data(), tris, n * sizeof(ctr_triangle), hipMemcpyDeviceToHost));
      host_tris = from_device.data();
    }
    tree = host_mesh_tree(host_tris, n);
    c.stamp("host build");
  }
  bool ok = tree.order.size() == n && !tree.nodes.empty();
  for (uint32_t k = 0; ok && k < n; k++) ok = tree.order[k] < n;
  if (!ok) return fail(CTR_E_INVALID, who + "the builder's tree is not one the refit can walk");
  const uint32_t count = (uint32_t)tree.nodes.size();
  std::unique_ptr<MeshRefit> refit;
  if (int st = refit_of_tree(tree.nodes.data(), count, n, who, refit)) return st;
  // where the mesh's ranges will live: a rebuild moves a tree that does not fit into exactly its room, a replace leaves room to grow
  // ... and an add takes the ranges that removed objects left behind before it lets the arrays grow
  ReplaceRoom room;
  if (c.adding) {
    const AddRoom ar = add_room(F, n, count);
    room = ReplaceRoom{ar.tris_reused, ar.nodes_reused, ar.tri_cap, ar.node_cap, ar.tris_after, ar.nodes4_after};
  } else {
    room = replace_room(F, c.gi, n, count, replace ? CTR_REPLACE_GROWTH : 1u);
  }
  if (room.tris_after > CTR_SCENE_TRIS_MAX)
    return fail(CTR_E_INVALID, who + std::to_string(room.tris_after) + " triangle records: more than the scene's arrays can address");
  const uint32_t n_before = c.adding ? 0u : F.guards[c.gi].tri_count;
  if (int st = s->upd_back.reserve(BackLayout(n, count).end)) return st;
  if (int st = s->rb_index.reserve(n)) return st;
  if (n != n_before && s->scan_planes.cap) {
    // the guard's scan on the device keeps every mesh's planes in one array, this mesh's in the middle of it: with another count
    // the array is laid out anew (the next scan uploads it whole), and it and the scan's words get their room here, not there.
    // (Scratch, not scene: should a later step fail, the cost is that upload.)
    const uint64_t planes_after = guard_plane_count(F) - n_before + n;
    s->scan_planes_live = false;
    if (int st = s->scan_planes.reserve(planes_after)) return st;
    if (int st = reserve_both(s->scan_words, s->scan_back, guard_scan_words(planes_after))) return st;
  }
  const size_t n_guards = F.guards.size() + (c.adding ? 1u : 0u);
  if (s->refit.size() < n_guards) s->refit.resize(n_guards);
  F.tris.reserve(room.tris_after);
  F.gn.reserve(4 * room.tris_after);
  F.nodes4.reserve(room.nodes4_after);
  if (c.adding) {
    F.objs.reserve(F.objs.size() + 1);
    F.guards.reserve(n_guards);
  } else {
    F.guards[c.gi].planes.reserve((size_t)CTR_PLANE_DOUBLES * n);
  }
  if (int st = c.edit.begin()) return st;  // (no launch may still be reading an array either, when it moves)
  if (c.adding) {
    // one object more, one mesh more in the top-level tree (a binary tree over m leaves has fewer than m nodes)
    size_t n_mesh = 1;
    for (const MeshGuard &g : F.guards) n_mesh += g.tri_count != 0;
    if (int st = s->d_objs.grow(F.objs.size() + 1, F.objs.size())) return st;
    if (int st = s->d_meshes.grow(n_mesh, F.meshes.size())) return st;
    if (int st = s->d_nodes.grow(2 * n_mesh, F.nodes.size())) return st;
  }
  // The same contents in another place (the DEVICE's, which for a linear mesh are not the host copy's): the last steps that can fail
  // for want of memory.  An array that grew before a later one failed holds what it held, at another address, and every launch
  // takes the addresses from the handle anew: harmless.
  const size_t tris_before = F.tris.size();
  if (int st = s->d_tris.grow(room.tris_after, tris_before)) return st;
  if (int st = s->d_gnorm.grow(room.tris_after, tris_before)) return st;
  if (int st = s->d_nodes4.grow(room.nodes4_after, F.nodes4.size())) return st;

  // ---- 1c. the shape goes in: host copy, then the device's descriptors and the records' `orig` ----
  bool nodes_moved = false, tris_moved = false;
  std::vector<DirtyRange> dirty;
  if (c.adding) {
    dirty = mesh_added(F, c.mat_idx, n, tree);
    c.gi = F.guards.size() - 1;
    tris_moved = room.tris_move;
    nodes_moved = room.nodes_move;
  } else {
    dirty = replace ? mesh_replaced(F, c.gi, n, tree, &tris_moved, &nodes_moved) : mesh_rebuilt(F, c.gi, tree, &nodes_moved);
  }
  s->refit[c.gi] = std::move(refit);
  if (int st = upload_dirty(s, dirty)) return st;
  HIP_TRY(hipMemcpyAsync(s->rb_index.p, tree.order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
  if (int st = launched(ctr_launch_set_orig(s->d_tris.as<DTri>() + F.guards[c.gi].tri_begin, s->rb_index.as<uint32_t>(), n, c.stream), "set_orig launch"))
    return st;
  if (c.stamp.on) HIP_TRY(hipStreamSynchronize(c.stream));
  c.stamp("install");

  // ---- 2. .. 5. the update's steps, with the new schedule ----
  if (int st = update_steps(c, s->refit[c.gi].get())) return st;
  built.node_count = count;
  built.levels = (uint32_t)s->refit[c.gi]->sched.levels();
  built.nodes_moved = nodes_moved ? 1u : 0u;
  built.tris_moved = tris_moved ? 1u : 0u;
  built.tri_cap = F.guards[c.gi].tri_cap;
  return CTR_OK;
}

}  // namespace

extern "C" {

int ctr_scene_update_mesh(ctr_scene *s, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, void *hip_stream) {
  if (!s || !tris) return fail(CTR_E_INVALID, "ctr_scene_update_mesh: null argument");
  MeshCall c(s, "ctr_scene_update_mesh");
  if (int st = mesh_arguments(c, object, tris, n_tris, hip_stream)) return st;
  MeshRefit *refit = nullptr;
  if (int st = mesh_refit_of(s, c.gi, &refit)) return st;
  if (int st = vertices_and_buffers(c, s->flat.guards[c.gi].node_count)) return st;
  if (int st = c.edit.begin()) return st;
  c.stamp("checks");
  return update_steps(c, refit);
}

int ctr_scene_rebuild_mesh(ctr_scene *s, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags, ctr_rebuild_info *info,
                           void *hip_stream) {
  const std::string who = "ctr_scene_rebuild_mesh: ";
  if (flags & ~CTR_REBUILD_HOST) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(flags & ~CTR_REBUILD_HOST));
  if (!s || !tris) return fail(CTR_E_INVALID, who + "null argument");
  MeshCall c(s, "ctr_scene_rebuild_mesh");
  Built built;
  if (int st = rebuild_or_replace(c, object, tris, n_tris, (flags & CTR_REBUILD_HOST) != 0, false, hip_stream, built)) return st;
  if (info) {
    *info = ctr_rebuild_info{};
    info->builder = built.builder;
    info->fell_back = built.fell_back;
    info->node_count = built.node_count;
    info->levels = built.levels;
    info->moved = built.nodes_moved;
  }
  return CTR_OK;
}

int ctr_scene_replace_mesh(ctr_scene *s, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags, ctr_replace_info *info,
                           void *hip_stream) {
  const std::string who = "ctr_scene_replace_mesh: ";
  if (flags & ~CTR_REPLACE_HOST) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(flags & ~CTR_REPLACE_HOST));
  if (!s || !tris) return fail(CTR_E_INVALID, who + "null argument");
  MeshCall c(s, "ctr_scene_replace_mesh");
  Built built;
  if (int st = rebuild_or_replace(c, object, tris, n_tris, (flags & CTR_REPLACE_HOST) != 0, true, hip_stream, built)) return st;
  if (info) *info = ctr_replace_info{built.builder, built.fell_back, built.node_count, built.levels, built.nodes_moved, built.tris_moved, built.tri_cap, 0u};
  return CTR_OK;
}

int ctr_scene_add_mesh(ctr_scene *s, uint64_t mat_idx, const ctr_triangle *tris, uint64_t n_tris, uint32_t flags, ctr_add_info *info, void *hip_stream) {
  const std::string who = "ctr_scene_add_mesh: ";
  if (flags & ~CTR_ADD_HOST) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(flags & ~CTR_ADD_HOST));
  if (!s || !tris) return fail(CTR_E_INVALID, who + "null argument");
  MeshCall c(s, "ctr_scene_add_mesh");
  if (int st = add_arguments(c, mat_idx, tris, n_tris, hip_stream)) return st;
  Built built;
  if (int st = rebuild_or_replace(c, 0, tris, n_tris, (flags & CTR_ADD_HOST) != 0, true, hip_stream, built)) return st;
  if (info)
    *info = ctr_add_info{s->flat.guards[c.gi].obj_index, built.builder, built.fell_back, built.node_count, built.levels, built.tris_moved, built.nodes_moved, built.tri_cap};
  return CTR_OK;
}

int ctr_scene_mesh_box(const ctr_scene *s, uint32_t object, ctr_vec3 *bb_min, ctr_vec3 *bb_max) {
  if (!s || !bb_min || !bb_max) return fail(CTR_E_INVALID, "ctr_scene_mesh_box: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  const FlatScene &F = s->flat;
  if (object >= F.objs.size() || F.objs[object].type != CTR_OBJ_MESH)
    return fail(CTR_E_INVALID, "ctr_scene_mesh_box: object #" + std::to_string(object) + " is not a mesh");
  const float *f = F.objs[object].f;
  *bb_min = ctr_vec3{f[0], f[1], f[2]};
  *bb_max = ctr_vec3{f[3], f[4], f[5]};
  return CTR_OK;
}

}  // extern "C"
