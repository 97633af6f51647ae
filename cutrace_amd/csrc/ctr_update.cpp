// ctr_update.cpp — the host half of include/cutrace_update.h: ctr_scene_update_mesh and ctr_scene_mesh_box.  No HIP kernels here:
// the device half is mesh_update.hip, the arithmetic both sides share is tri_record.h and mesh_refit.h.
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
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "ctr_internal.h"
#include "cutrace_update.h"
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

// the mesh's level schedule, on the host and on the device, from the host copy of its tree: once per mesh
int mesh_refit_of(ctr_scene *s, size_t gi, MeshRefit **out) {
  if (s->refit.size() < s->flat.guards.size()) s->refit.resize(s->flat.guards.size());
  if (!s->refit[gi]) {
    const FlatScene &F = s->flat;
    const MeshGuard &g = F.guards[gi];
    auto r = std::make_unique<MeshRefit>();
    bool ok = level_schedule(&F.nodes4[g.node_begin], g.node_count, g.tri_count, r->sched);
    // (the kernels index the caller's vertices by a record's `orig`: it must name a triangle of the mesh)
    for (uint32_t k = 0; ok && k < g.tri_count; k++) ok = F.tris[g.tri_begin + k].orig < g.tri_count;
    if (!ok) return fail(CTR_E_INVALID, "ctr_scene_update_mesh: the mesh's tree is not one the refit can walk");
    if (int st = r->d_nodes.reserve(r->sched.nodes.size())) return st;
    HIP_TRY(hipMemcpy(r->d_nodes.p, r->sched.nodes.data(), r->sched.nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    s->refit[gi] = std::move(r);
  }
  *out = s->refit[gi].get();
  return CTR_OK;
}

// CUTRACE_DEBUG_UPDATE=1: where ctr_scene_update_mesh spends its time (stderr), the time since the previous stamp; the device
// kernels then get a wait of their own, so that their time is not counted as the copy-back's (scripts/gpu_mesh_update.py)
struct Stamps {
  const bool on = getenv("CUTRACE_DEBUG_UPDATE") != nullptr;
  std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::high_resolution_clock::now();
    fprintf(stderr, "cutrace_amd update_mesh: %-24s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
    t0 = now;
  }
};

}  // namespace

extern "C" {

int ctr_scene_update_mesh(ctr_scene *s, uint32_t object, const ctr_triangle *tris, uint64_t n_tris, void *hip_stream) {
  const std::string who = "ctr_scene_update_mesh: ";
  if (!s || !tris) return fail(CTR_E_INVALID, who + "null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  FlatScene &F = s->flat;
  if (object >= F.objs.size() || F.objs[object].type != CTR_OBJ_MESH)
    return fail(CTR_E_INVALID, who + "object #" + std::to_string(object) + " is not a mesh");
  if (F.objs[object].tri_count == 0) return fail(CTR_E_INVALID, who + "object #" + std::to_string(object) + " is an empty mesh");
  if (n_tris != F.objs[object].tri_count)
    return fail(CTR_E_INVALID, who + std::to_string(n_tris) + " triangles for a mesh of " + std::to_string(F.objs[object].tri_count) +
                                   ": the count is fixed");
  size_t gi = 0;
  while (gi < F.guards.size() && F.guards[gi].obj_index != object) gi++;
  if (gi == F.guards.size() || F.guards[gi].mesh_pos < 0) return fail(CTR_E_INVALID, who + "the mesh has no records");
  const uint32_t n = (uint32_t)n_tris;
  const uint32_t tri_begin = F.guards[gi].tri_begin, node_begin = F.guards[gi].node_begin, node_count = F.guards[gi].node_count;

  Stamps stamp;
  if (int st = use_device(s)) return st;
  const Where where = where_is(tris, n * sizeof(ctr_triangle), s->device);
  if (where == Where::ELSEWHERE) return fail(CTR_E_INVALID, who + "tris is neither host memory nor device memory of the scene's device");
  hipStream_t stream = (hipStream_t)hip_stream;

  // ---- 1. the vertices must be finite; buffers (nothing of the scene changes yet) ----
  MeshRefit *refit = nullptr;
  if (int st = mesh_refit_of(s, gi, &refit)) return st;
  const size_t b_tris = 0, b_gn = b_tris + align16(n * sizeof(DTri)), b_nodes = b_gn + align16(n * 4 * sizeof(float)),
               b_planes = b_nodes + align16(node_count * sizeof(DNode4)), b_box = b_planes + align16(n * CTR_PLANE_DOUBLES * sizeof(double)),
               b_flag = b_box + 32, b_end = b_flag + 16;
  if (int st = s->upd_back.reserve(b_end)) return st;
  if (int st = s->upd_planes.reserve(n)) return st;
  if (int st = s->upd_words.reserve(8)) return st;
  char *back = s->upd_back.as<char>();
  uint32_t *d_flag = s->upd_words.as<uint32_t>();
  float *d_box = s->upd_words.as<float>() + 2;
  const float *d_verts = (const float *)tris;
  if (where == Where::HOST) {
    const float *v = (const float *)tris;
    for (size_t i = 0; i < 9 * (size_t)n; i++)
      if (!std::isfinite(v[i])) return fail(CTR_E_INVALID, who + "triangle " + std::to_string(i / 9) + " has a vertex that is not finite");
    if (int st = s->upd_verts.reserve(n)) return st;
    d_verts = s->upd_verts.as<float>();
  } else {
    // a small kernel of its own, its one flag word read back before anything is modified
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), stream));
    if (int st = launched(ctr_launch_all_finite(d_verts, 9 * (uint64_t)n, d_flag, stream), "finiteness check launch")) return st;
    HIP_TRY(hipMemcpyAsync(back + b_flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    uint32_t flag;
    memcpy(&flag, back + b_flag, sizeof(flag));
    if (flag) return fail(CTR_E_INVALID, who + "a vertex is not finite");
  }

  // ---- 2. the device side, on the caller's stream ----
  HIP_TRY(hipDeviceSynchronize());  // no launch may still be reading the old records (as ctr_scene_set_cameras does)
  stamp("checks");
  if (where == Where::HOST) HIP_TRY(hipMemcpyAsync(s->upd_verts.p, tris, n * sizeof(ctr_triangle), hipMemcpyHostToDevice, stream));
  DTri *d_recs = const_cast<DTri *>(s->dev.tris) + tri_begin;
  float *d_gn = const_cast<float *>(s->dev.gnorm) + 4 * (size_t)tri_begin;
  DNode4 *d_nodes = (DNode4 *)const_cast<void *>(s->dev.nodes4) + node_begin;  // (the mesh's spare node and guard records are not the kernels' business)
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
  HIP_TRY(hipMemcpyAsync(back + b_tris, d_recs, n * sizeof(DTri), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b_gn, d_gn, n * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b_nodes, d_nodes, node_count * sizeof(DNode4), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b_planes, d_planes, n * CTR_PLANE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(back + b_box, d_box, 6 * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  MeshGuard &g = F.guards[gi];
  memcpy(&F.tris[tri_begin], back + b_tris, n * sizeof(DTri));
  memcpy(&F.gn[4 * (size_t)tri_begin], back + b_gn, n * 4 * sizeof(float));
  memcpy(&F.nodes4[node_begin], back + b_nodes, node_count * sizeof(DNode4));
  memcpy(g.planes.data(), back + b_planes, n * CTR_PLANE_DOUBLES * sizeof(double));
  float box[6];
  memcpy(box, back + b_box, sizeof(box));
  stamp("copy-back");

  // ---- 4., 5. everything derived from them, then the guard ----
  if (int st = upload_dirty(s, mesh_updated(F, gi, box))) return st;
  stamp("host records + upload");
  // (the new planes are on the device already, in upd_planes, and the stream has been waited for: the scan takes them from there)
  if (int st = guard_planes_changed(s, gi, d_planes)) return st;
  const int st = refresh_linear_meshes(s, true);
  stamp("guard");
  return st;
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
