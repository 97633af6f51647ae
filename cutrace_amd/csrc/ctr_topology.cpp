// ctr_topology.cpp — include/cutrace_topology.h: ctr_scene_add_object, ctr_scene_remove_object and ctr_scene_room.  ctr_scene_add_mesh
// is ctr_update.cpp's: its device work is a replace's, on a range of its own.
// No HIP kernels here: the surgery on the host copy is scene_flatten.cpp's (object_added, object_removed: the text flatten_scene
// runs), the guard is guard.cpp's, and its plane scan on the device is guard_scan.hip.
//
// An edit of the list in four steps, ctr_edit.cpp's:
//   1. the arguments are checked as validate_desc checks a description; nothing of the handle has changed when the call fails here
//   2. the device is waited for, and every device array the edit can outgrow gets its room (contents kept)
//   3. the host copy is edited; the device receives every array that holds one record per object, plane pair, mesh or top-level node
//   4. refresh_linear_meshes: a flat object that reflects is a mirror, and the eyes' images come and go with it
// What the handle indexes by MeshGuard follows the list: the refit schedules, and the device scan's flat plane array, which is
// laid out anew at the next scan.
#include <hip/hip_runtime_api.h>

#include <mutex>
#include <string>

#include "ctr_internal.h"
#include "cutrace_topology.h"

namespace {
size_t plane_count(const FlatScene &F) {
  size_t n = 0;
  for (const DObj &O : F.objs) n += O.type == CTR_OBJ_PLANE;
  return n;
}
}  // namespace

extern "C" {

int ctr_scene_add_object(ctr_scene *s, const ctr_object *object, uint64_t *index) {
  const std::string who = "ctr_scene_add_object: ";
  if (!s || !object) return fail(CTR_E_INVALID, who + "null argument");
  const Edit edit(s);
  FlatScene &F = s->flat;
  std::string err;
  if (int st = check_new_object(F, *object, err)) return fail(st, who + err);
  const bool tri = object->type == CTR_OBJ_TRIANGLE;
  bool record_free = false;
  for (const FlatScene::FreeRange &r : F.free_tris) record_free |= r.count == 1;
  const size_t tris_after = F.tris.size() + (tri && !record_free ? 1u : 0u);
  if (tris_after > CTR_SCENE_TRIS_MAX) return fail(CTR_E_INVALID, who + std::to_string(tris_after) + " triangle records: more than the scene's arrays can address");
  const size_t planes_after = plane_count(F) + (object->type == CTR_OBJ_PLANE ? 1u : 0u);
  F.objs.reserve(F.objs.size() + 1);
  F.oloop.reserve(F.oloop.size() + 1);
  F.tris.reserve(tris_after);
  F.gn.reserve(4 * tris_after);
  if (int st = edit.begin()) return st;
  if (int st = s->d_objs.grow(F.objs.size() + 1, F.objs.size())) return st;
  if (int st = s->d_oloop.grow(F.oloop.size() + 1, F.oloop.size())) return st;
  if (int st = s->d_planes.grow(plane_records_at_most(planes_after), F.planes.size())) return st;
  if (int st = s->d_tris.grow(tris_after, F.tris.size())) return st;
  if (int st = s->d_gnorm.grow(tris_after, F.tris.size())) return st;
  const std::vector<DirtyRange> dirty = object_added(F, *object);
  // (holds while plane_records_at_most does; nothing is uploaded past the end of the array whatever that function says)
  if (F.planes.size() > s->d_planes.cap) return fail(CTR_E_INVALID, who + "more plane records than plane_records_at_most allows");
  if (index) *index = F.objs.size() - 1;
  return edit.end(dirty, true);
}

int ctr_scene_remove_object(ctr_scene *s, uint64_t index) {
  const std::string who = "ctr_scene_remove_object: ";
  if (!s) return fail(CTR_E_INVALID, who + "null argument");
  const Edit edit(s);
  FlatScene &F = s->flat;
  if (index >= F.objs.size()) return fail(CTR_E_INVALID, who + "object #" + std::to_string(index) + " out of range");
  const uint32_t type = F.objs[index].type;
  const size_t planes_after = plane_count(F) - (type == CTR_OBJ_PLANE ? 1u : 0u);
  if (type == CTR_OBJ_TRIANGLE) F.free_tris.reserve(F.free_tris.size() + 1);
  if (type == CTR_OBJ_MESH) {
    F.free_tris.reserve(F.free_tris.size() + 1);
    F.free_nodes4.reserve(F.free_nodes4.size() + 1);
  }
  if (int st = edit.begin()) return st;
  // (fewer planes can need MORE records: five walls are one triple, two of them on one axis a general pair — and four of them two triples)
  if (int st = s->d_planes.grow(plane_records_at_most(planes_after), F.planes.size())) return st;
  long gi = -1;
  const std::vector<DirtyRange> dirty = object_removed(F, index, &gi);
  if (gi >= 0) {
    if ((size_t)gi < s->refit.size()) s->refit.erase(s->refit.begin() + gi);
    s->scan_planes_live = false;  // (laid out in guards order; it only shrinks, so its room and the words' are there)
  }
  if (F.planes.size() > s->d_planes.cap) return fail(CTR_E_INVALID, who + "more plane records than plane_records_at_most allows");
  // (a top-level tree over fewer meshes has fewer nodes: nothing is uploaded past the end of an array whatever the builder does)
  if (F.nodes.size() > s->d_nodes.cap || F.meshes.size() > s->d_meshes.cap) return fail(CTR_E_INVALID, who + "a larger top-level tree than its arrays have room for");
  return edit.end(dirty, true);
}

int ctr_scene_room(const ctr_scene *s, struct ctr_scene_room *out) {
  if (!s || !out) return fail(CTR_E_INVALID, "ctr_scene_room: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  const SceneRoom r = scene_room(s->flat);
  *out = {r.tris_live, r.tris_total, r.nodes4_live, r.nodes4_total};
  return CTR_OK;
}

}  // extern "C"
