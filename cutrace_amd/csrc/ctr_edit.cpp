// ctr_edit.cpp — include/cutrace_edit.h: ctr_scene_set_lights, ctr_scene_set_materials, the two counts and ctr_debug_guard_state;
// include/cutrace_objects.h: ctr_scene_set_objects, ctr_scene_object_count, ctr_scene_get_object.
// No HIP kernels here: the records and flags are scene_flatten.cpp's (light_records, material_records, objects_edited: the text
// flatten_scene runs), the guard is guard.cpp's, and its plane scan on the device is guard_scan.hip.
//
// An edit in four steps:
//   1. the arguments are checked as validate_desc checks a description; nothing of the handle has changed when the call fails here
//   2. the device is waited for, and the device array gets room for the new count (reused when it fits)
//   3. the host copy gets the records, the flags and — materials, objects — the objects' transparency bits; the device receives them
//   4. refresh_linear_meshes: the lights are probes of the guard, a reflecting material makes mirrors, a flat object that
//      reflects is one and moves the eyes' images with it
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "ctr_internal.h"
#include "cutrace_edit.h"

extern "C" {

int ctr_scene_set_lights(ctr_scene *s, const ctr_light *lights, uint64_t n) {
  const std::string who = "ctr_scene_set_lights: ";
  if (!s || (!lights && n)) return fail(CTR_E_INVALID, who + "null argument");
  for (uint64_t i = 0; i < n; i++)
    if (lights[i].type > CTR_LIGHT_POINT) return fail(CTR_E_INVALID, who + "light #" + std::to_string(i) + ": bad type");
  const Edit edit(s);
  FlatScene &F = s->flat;
  if (int st = edit.begin()) return st;
  if (int st = s->d_lights.grow(n, 0)) return st;
  light_records(F, lights, n);
  if (n) HIP_TRY(hipMemcpy(s->d_lights.p, F.lights.data(), n * sizeof(DLight), hipMemcpyHostToDevice));
  return edit.end({}, true);
}

int ctr_scene_set_materials(ctr_scene *s, const ctr_material *mats, uint64_t n) {
  const std::string who = "ctr_scene_set_materials: ";
  if (!s || (!mats && n)) return fail(CTR_E_INVALID, who + "null argument");
  for (uint64_t i = 0; i < n; i++)
    if (mats[i].type != CTR_MAT_PHONG) return fail(CTR_E_INVALID, who + "material #" + std::to_string(i) + ": bad type");
  const Edit edit(s);
  FlatScene &F = s->flat;
  for (size_t i = 0; i < F.objs.size(); i++)
    if (F.objs[i].mat >= n) return fail(CTR_E_INVALID, who + "object #" + std::to_string(i) + ": material index out of range");
  if (int st = edit.begin()) return st;
  if (int st = s->d_mats.grow(n, 0)) return st;
  const std::vector<DirtyRange> dirty = material_records(F, mats, n);
  if (n) HIP_TRY(hipMemcpy(s->d_mats.p, F.mats.data(), n * sizeof(DMat), hipMemcpyHostToDevice));
  return edit.end(dirty, true);
}

int ctr_scene_set_objects(ctr_scene *s, const ctr_object *objects, uint64_t n) {
  const std::string who = "ctr_scene_set_objects: ";
  if (!s) return fail(CTR_E_INVALID, who + "null argument");
  const Edit edit(s);
  FlatScene &F = s->flat;
  std::string err;
  if (int st = check_objects(F, objects, n, err)) return fail(st, who + err);
  if (int st = edit.begin()) return st;
  // (room for the most records ANY packing of these planes needs: the count after the edit is known only once the host copy has it)
  if (int st = s->d_planes.grow(plane_records_at_most(F), 0)) return st;
  const std::vector<DirtyRange> dirty = objects_edited(F, objects, n);
  // (holds while plane_records_at_most does; nothing is uploaded past the end of the array whatever that function says)
  if (F.planes.size() > s->d_planes.cap) return fail(CTR_E_INVALID, who + "more plane records than plane_records_at_most allows");
  return edit.end(dirty, true);
}

int ctr_scene_object_count(const ctr_scene *s, uint64_t *n) {
  if (!s || !n) return fail(CTR_E_INVALID, "ctr_scene_object_count: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  *n = s->flat.objs.size();
  return CTR_OK;
}

int ctr_scene_get_object(const ctr_scene *s, uint64_t index, ctr_object *out) {
  if (!s || !out) return fail(CTR_E_INVALID, "ctr_scene_get_object: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  if (index >= s->flat.objs.size()) return fail(CTR_E_INVALID, "ctr_scene_get_object: object #" + std::to_string(index) + " out of range");
  *out = object_of(s->flat, index);
  return CTR_OK;
}

int ctr_scene_light_count(const ctr_scene *s, uint64_t *n) {
  if (!s || !n) return fail(CTR_E_INVALID, "ctr_scene_light_count: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  *n = s->flat.lights.size();
  return CTR_OK;
}

int ctr_scene_material_count(const ctr_scene *s, uint64_t *n) {
  if (!s || !n) return fail(CTR_E_INVALID, "ctr_scene_material_count: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ctr_scene *>(s)->mtx);
  *n = s->flat.mats.size();
  return CTR_OK;
}

int ctr_debug_guard_state(ctr_scene *s, uint32_t object, uint32_t *guarded, uint64_t capacity, uint64_t *n_guarded, int *linear) {
  if (!s || !n_guarded || !linear || (!guarded && capacity)) return fail(CTR_E_INVALID, "ctr_debug_guard_state: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  const FlatScene &F = s->flat;
  if (object >= F.objs.size() || F.objs[object].type != CTR_OBJ_MESH)
    return fail(CTR_E_INVALID, "ctr_debug_guard_state: object #" + std::to_string(object) + " is not a mesh");
  *n_guarded = 0;
  *linear = 0;
  for (const MeshGuard &g : F.guards) {
    if (g.obj_index != object || g.mesh_pos < 0) continue;
    std::vector<uint32_t> file;
    for (uint32_t t : g.guarded) file.push_back(F.tris[g.tri_begin + t].orig);
    std::sort(file.begin(), file.end());
    *n_guarded = file.size();
    *linear = g.linear ? 1 : 0;
    for (uint64_t k = 0; k < file.size() && k < capacity; k++) guarded[k] = file[k];
  }
  return CTR_OK;
}

}  // extern "C"
