// ctr_rays.cpp — the C-ABI of include/cutrace_rays.h: ctr_cast_rays, ctr_shade_rays and ctr_shade_points check a query,
// describe the uploaded scene to the kernel (RayScene, ray_query.h) and launch it (ray_query.hip, ray_shade.hip, ray_points.hip).
#include <hip/hip_runtime_api.h>

#include <string>

#include "ctr_internal.h"
#include "cutrace_rays.h"
#include "ray_points.h"
#include "ray_query.h"
#include "ray_shade.h"

namespace {

// what both queries check after their own flags and outputs: the scene, the number of rays and, when there are any, the rays
int check_rays(const ctr_scene *s, const std::string &who, uint64_t n_rays, const float *d_origin, const float *d_dir) {
  if (!s) return fail(CTR_E_INVALID, who + "null scene");
  if (n_rays >= 0x80000000ull) return fail(CTR_E_INVALID, who + "n_rays must be below 2^31");
  if (n_rays && (!d_origin || !d_dir)) return fail(CTR_E_INVALID, who + "null rays");
  return CTR_OK;
}

}  // namespace

// every pointer the kernel touches must be device memory of the scene's device (no size check is possible here)
// (ctr_internal.h: the lens render checks its ray arrays with it, ctr_quantise_device its planes)
int check_device_pointers(int device, const std::string &who, const void *const *ptrs, const char *const *names, size_t n,
                          const char *whose) {
  for (size_t k = 0; k < n; k++) {
    if (!ptrs[k]) continue;
    hipPointerAttribute_t at{};
    const bool ok = hipPointerGetAttributes(&at, ptrs[k]) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device;
    if (!ok) {
      (void)hipGetLastError();  // plain host memory: "invalid value", not an error of the stream
      return fail(CTR_E_INVALID, who + names[k] + " is not device memory of " + whose);
    }
  }
  return CTR_OK;
}

namespace {

// what the walk of ray_walk.h needs of the scene on the device (ctr_internal.h device_scene)
RayScene ray_scene(const ctr_scene *s, const DScene &D) {
  return {D.objs, D.oloop, D.meshes, D.planes, D.tris, D.nodes4, D.gnorm, D.mats, D.n_oloop, D.n_plane_recs, D.n_mesh, s->flat.ray_slots};
}

}  // namespace

extern "C" int ctr_cast_rays(ctr_scene *s, const ctr_ray_query *q, void *hip_stream) {
  const std::string who = "ctr_cast_rays: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  constexpr uint32_t KNOWN = CTR_RAY_IGNORE_TRANSPARENT | CTR_RAY_LINEAR | CTR_RAY_SHADOW;
  if (q->flags & ~KNOWN) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(q->flags & ~KNOWN));
  const bool shadow = (q->flags & CTR_RAY_SHADOW) != 0;
  const bool any_nearest = q->d_t || q->d_object || q->d_prim || q->d_point || q->d_normal || q->d_uv;
  if (shadow && (q->flags & CTR_RAY_IGNORE_TRANSPARENT))
    return fail(CTR_E_INVALID, who + "CTR_RAY_SHADOW and CTR_RAY_IGNORE_TRANSPARENT exclude each other");
  if (shadow && (any_nearest || !q->d_shadow))
    return fail(CTR_E_INVALID, who + "CTR_RAY_SHADOW writes d_shadow only, and needs it");
  if (!shadow && (!any_nearest || q->d_shadow))
    return fail(CTR_E_INVALID, who + "a nearest-hit query needs at least one of its outputs and no d_shadow");
  if (int st = check_rays(s, who, q->n_rays, q->d_origin, q->d_dir)) return st;
  if (q->n_rays == 0) return CTR_OK;
  const void *ptrs[] = {q->d_origin, q->d_dir, q->d_min_t, q->d_max_t, q->d_t, q->d_object, q->d_prim, q->d_point,
                        q->d_normal, q->d_uv, q->d_shadow};
  const char *names[] = {"d_origin", "d_dir", "d_min_t", "d_max_t", "d_t", "d_object", "d_prim", "d_point",
                         "d_normal", "d_uv", "d_shadow"};
  if (int st = check_device_pointers(s->device, who, ptrs, names, sizeof(ptrs) / sizeof(ptrs[0]))) return st;
  if (int st = use_device(s)) return st;
  RayLaunch L{};
  L.scene = ray_scene(s, device_scene(s));
  L.n_rays = (uint32_t)q->n_rays;
  L.flags = q->flags;
  L.anyhit = shadow && s->flat.all_opaque;
  L.min_t = q->min_t;
  L.max_t = q->max_t;
  L.origin = q->d_origin;
  L.dir = q->d_dir;
  L.min_t_arr = q->d_min_t;
  L.max_t_arr = q->d_max_t;
  L.t = q->d_t;
  L.object = q->d_object;
  L.prim = q->d_prim;
  L.point = q->d_point;
  L.normal = q->d_normal;
  L.uv = q->d_uv;
  L.shadow = q->d_shadow;
  const int e = ctr_launch_rays(L, hip_stream);
  if (e) return hip_fail((hipError_t)e, "ray query kernel launch");
  return CTR_OK;
}

extern "C" int ctr_shade_rays(ctr_scene *s, const ctr_shade_query *q, void *hip_stream) {
  const std::string who = "ctr_shade_rays: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  constexpr uint32_t KNOWN = CTR_SHADE_LINEAR | CTR_SHADE_EXACT_POW;
  if (q->flags & ~KNOWN) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(q->flags & ~KNOWN));
  if (q->bounces < 0 || q->bounces > CTR_MAX_BOUNCES)
    return fail(CTR_E_INVALID, who + "bounces " + std::to_string(q->bounces) + " outside [0, " + std::to_string(CTR_MAX_BOUNCES) + "]");
  if (!q->d_color) return fail(CTR_E_INVALID, who + "d_color is required");
  if (int st = check_rays(s, who, q->n_rays, q->d_origin, q->d_dir)) return st;
  if (q->n_rays == 0) return CTR_OK;
  const void *ptrs[] = {q->d_origin, q->d_dir, q->d_color, q->d_t, q->d_object, q->d_normal};
  const char *names[] = {"d_origin", "d_dir", "d_color", "d_t", "d_object", "d_normal"};
  if (int st = check_device_pointers(s->device, who, ptrs, names, sizeof(ptrs) / sizeof(ptrs[0]))) return st;
  const DScene D = device_scene(s);
  ShadeLaunch L{};
  L.scene = ray_scene(s, D);
  L.lights = D.lights;
  L.n_light = D.n_light;
  L.frames = ctr_shade_frames(q->bounces, s->flat.any_bounce);
  L.frame_dwords = s->flat.need_cold ? 10u : 4u;
  L.all_opaque = s->flat.all_opaque ? 1u : 0u;
  L.n_rays = (uint32_t)q->n_rays;
  L.flags = q->flags | (s->flat.fast_pow_ok ? 0u : CTR_SHADE_EXACT_POW);  // (outside the fast path's domain: the exact one)
  L.bounces = q->bounces;
  L.min_t = q->min_t;
  L.ambient = q->ambient;
  L.origin = q->d_origin;
  L.dir = q->d_dir;
  L.color = q->d_color;
  L.t = q->d_t;
  L.object = q->d_object;
  L.normal = q->d_normal;
  if (ctr_shade_lds_bytes(L) > CTR_SHADE_LDS_MAX)
    return fail(CTR_E_INVALID, who + "the walk stack of this scene's mesh trees and " + std::to_string(L.frames) +
                                   " recursion frames need " + std::to_string(ctr_shade_lds_bytes(L)) +
                                   " bytes of LDS per workgroup, more than " + std::to_string(CTR_SHADE_LDS_MAX) +
                                   " (fewer bounces or CTR_SHADE_LINEAR fit)");
  if (int st = use_device(s)) return st;
  const int e = ctr_launch_shade(L, hip_stream);
  if (e) return hip_fail((hipError_t)e, "radiance query kernel launch");
  return CTR_OK;
}

extern "C" int ctr_shade_points(ctr_scene *s, const ctr_point_query *q, void *hip_stream) {
  const std::string who = "ctr_shade_points: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  constexpr uint32_t KNOWN = CTR_POINTS_LINEAR | CTR_POINTS_EXACT_POW;
  if (q->flags & ~KNOWN) return fail(CTR_E_INVALID, who + "unknown flag bits " + std::to_string(q->flags & ~KNOWN));
  if (!q->d_color && !q->d_light_shadow) return fail(CTR_E_INVALID, who + "no output: one of d_color and d_light_shadow is required");
  if (q->d_color && (!q->d_normal || !q->d_view)) return fail(CTR_E_INVALID, who + "d_color needs d_normal and d_view");
  if (q->d_material && q->d_object) return fail(CTR_E_INVALID, who + "d_material and d_object exclude each other");
  if (!s) return fail(CTR_E_INVALID, who + "null scene");
  if (q->n_points >= 0x80000000ull) return fail(CTR_E_INVALID, who + "n_points must be below 2^31");
  if (q->n_points && !q->d_point) return fail(CTR_E_INVALID, who + "null d_point");
  const size_t n_mat = s->flat.mats.size();
  if (q->d_color && !q->d_material && !q->d_object && (q->material < 0 || (size_t)q->material >= n_mat))
    return fail(CTR_E_INVALID, who + "material " + std::to_string(q->material) + " outside [0, " + std::to_string(n_mat) + ")");
  if (q->n_points == 0) return CTR_OK;
  const void *ptrs[] = {q->d_point, q->d_normal, q->d_view, q->d_material, q->d_object, q->d_color, q->d_light_shadow};
  const char *names[] = {"d_point", "d_normal", "d_view", "d_material", "d_object", "d_color", "d_light_shadow"};
  if (int st = check_device_pointers(s->device, who, ptrs, names, sizeof(ptrs) / sizeof(ptrs[0]))) return st;
  const DScene D = device_scene(s);
  PointsLaunch L{};
  L.scene = ray_scene(s, D);
  L.lights = D.lights;
  L.n_light = D.n_light;
  L.n_mat = D.n_mat;
  L.n_obj = D.n_obj;
  L.all_opaque = s->flat.all_opaque ? 1u : 0u;
  L.n_points = (uint32_t)q->n_points;
  L.flags = q->flags | (s->flat.fast_pow_ok ? 0u : CTR_POINTS_EXACT_POW);  // (outside the fast path's domain: the exact one)
  L.material = q->material;
  L.ambient = q->ambient;
  L.point = q->d_point;
  // without d_color the kernel reads none of these
  L.normal = q->d_color ? q->d_normal : nullptr;
  L.view = q->d_color ? q->d_view : nullptr;
  L.mat_arr = q->d_color ? q->d_material : nullptr;
  L.obj_arr = q->d_color ? q->d_object : nullptr;
  L.color = q->d_color;
  L.light_shadow = L.n_light ? q->d_light_shadow : nullptr;
  if (ctr_points_lds_bytes(L) > CTR_POINTS_LDS_MAX)
    return fail(CTR_E_INVALID, who + "the walk stack of this scene's mesh trees needs " + std::to_string(ctr_points_lds_bytes(L)) +
                                   " bytes of LDS per workgroup, more than " + std::to_string(CTR_POINTS_LDS_MAX) +
                                   " (CTR_POINTS_LINEAR needs none)");
  if (!L.color && !L.light_shadow) return CTR_OK;  // a scene without lights: the rows of d_light_shadow are empty
  if (int st = use_device(s)) return st;
  const int e = ctr_launch_points(L, hip_stream);
  if (e) return hip_fail((hipError_t)e, "surface shading kernel launch");
  return CTR_OK;
}
