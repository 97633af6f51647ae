// ctr_rays.cpp — the C-ABI of include/cutrace_rays.h, include/cutrace_hits.h, include/cutrace_nearest.h and include/cutrace_inside.h:
// ctr_cast_rays, ctr_shade_rays, ctr_shade_points, ctr_list_hits, ctr_nearest_points, ctr_count_crossings and ctr_inside_points check a
// query, describe the uploaded scene to the kernel (RayScene, ray_query.h) and launch it (ray_query.hip, ray_shade.hip, ray_points.hip,
// ray_hits.hip, ray_nearest.hip, ray_cross.hip).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <string>

#include "ctr_internal.h"
#include "cutrace_hits.h"
#include "cutrace_inside.h"
#include "cutrace_nearest.h"
#include "cutrace_rays.h"
#include "ray_cross.h"
#include "ray_hits.h"
#include "ray_nearest.h"
#include "ray_points.h"
#include "ray_query.h"
#include "ray_shade.h"

namespace {

// What the entry points check alike, once the query is known not to be null: the record of one call.
struct QueryHead {
  const std::string &who;   // "ctr_...: ", the prefix of every message
  uint32_t flags, known;    // the query's flag word, the bits its entry point knows
  std::string broken;       // the first rule of the entry point's own (outputs, bounces) that the query breaks; empty: none
  uint64_t count;           // rays or points, and what the header calls the field
  const char *count_name;
  bool inputs;              // are the arrays every element is read from all there?  What to say when not
  const char *no_inputs;
};

// The checks in the order every entry point makes them: flag bits, its own rules, the scene, the count, the inputs.
int check_query(const ctr_scene *s, const QueryHead &h) {
  if (h.flags & ~h.known) return fail(CTR_E_INVALID, h.who + "unknown flag bits " + std::to_string(h.flags & ~h.known));
  if (!h.broken.empty()) return fail(CTR_E_INVALID, h.who + h.broken);
  if (!s) return fail(CTR_E_INVALID, h.who + "null scene");
  if (h.count >= 0x80000000ull) return fail(CTR_E_INVALID, h.who + h.count_name + " must be below 2^31");
  if (h.count && !h.inputs) return fail(CTR_E_INVALID, h.who + h.no_inputs);
  return CTR_OK;
}

// what the walk of ray_walk.h needs of the scene on the device (ctr_internal.h device_scene)
RayScene ray_scene(const ctr_scene *s, const DScene &D) {
  return {D.objs, D.oloop, D.meshes, D.planes, D.tris, D.nodes4, D.gnorm, D.mats, D.n_oloop, D.n_plane_recs, D.n_mesh, s->flat.ray_slots};
}

// what ShadeLaunch and PointsLaunch have in common: the scene, its lights, and the query's flags with `exact_pow` forced for
// a scene outside the fast specular path's domain.  Returns the device scene for what else the caller needs of it.
template <class Launch>
DScene fill_lit(Launch &L, const ctr_scene *s, uint32_t flags, uint32_t exact_pow) {
  const DScene D = device_scene(s);
  L.scene = ray_scene(s, D);
  L.lights = D.lights;
  L.n_light = D.n_light;
  L.all_opaque = s->flat.all_opaque ? 1u : 0u;
  L.flags = flags | (s->flat.fast_pow_ok ? 0u : exact_pow);
  return D;
}

// CTR_E_INVALID "<who><what> <bytes> bytes of LDS per workgroup, more than <most> (<way_out>)"
int lds_fail(const std::string &who, const std::string &what, size_t bytes, size_t most, const char *way_out) {
  return fail(CTR_E_INVALID, who + what + " " + std::to_string(bytes) + " bytes of LDS per workgroup, more than " + std::to_string(most) +
                                 " (" + way_out + ")");
}

// CTR_E_INVALID "<who>object <i> outside [-1, <objects>)" unless `object` is -1 or names an object of the scene
int check_object(const ctr_scene *s, const std::string &who, int32_t object) {
  const size_t n_obj = s->flat.objs.size();
  if (object < -1 || (object >= 0 && (size_t)object >= n_obj))
    return fail(CTR_E_INVALID, who + "object " + std::to_string(object) + " outside [-1, " + std::to_string(n_obj) + ")");
  return CTR_OK;
}

}  // namespace

extern "C" int ctr_cast_rays(ctr_scene *s, const ctr_ray_query *q, void *hip_stream) {
  const std::string who = "ctr_cast_rays: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  const bool shadow = (q->flags & CTR_RAY_SHADOW) != 0;
  const bool any_nearest = q->d_t || q->d_object || q->d_prim || q->d_point || q->d_normal || q->d_uv;
  const char *broken = "";
  if (shadow && (q->flags & CTR_RAY_IGNORE_TRANSPARENT)) broken = "CTR_RAY_SHADOW and CTR_RAY_IGNORE_TRANSPARENT exclude each other";
  else if (shadow && (any_nearest || !q->d_shadow)) broken = "CTR_RAY_SHADOW writes d_shadow only, and needs it";
  else if (!shadow && (!any_nearest || q->d_shadow)) broken = "a nearest-hit query needs at least one of its outputs and no d_shadow";
  if (int st = check_query(s, {who, q->flags, CTR_RAY_IGNORE_TRANSPARENT | CTR_RAY_LINEAR | CTR_RAY_SHADOW, broken, q->n_rays, "n_rays",
                               q->d_origin && q->d_dir, "null rays"}))
    return st;
  if (q->n_rays == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_origin, "d_origin"}, {q->d_dir, "d_dir"}, {q->d_min_t, "d_min_t"}, {q->d_max_t, "d_max_t"},
                           {q->d_t, "d_t"}, {q->d_object, "d_object"}, {q->d_prim, "d_prim"}, {q->d_point, "d_point"},
                           {q->d_normal, "d_normal"}, {q->d_uv, "d_uv"}, {q->d_shadow, "d_shadow"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
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
  return launched(ctr_launch_rays(L, hip_stream), "ray query kernel launch");
}

extern "C" int ctr_shade_rays(ctr_scene *s, const ctr_shade_query *q, void *hip_stream) {
  const std::string who = "ctr_shade_rays: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  std::string broken;
  if (q->bounces < 0 || q->bounces > CTR_MAX_BOUNCES)
    broken = "bounces " + std::to_string(q->bounces) + " outside [0, " + std::to_string(CTR_MAX_BOUNCES) + "]";
  else if (!q->d_color) broken = "d_color is required";
  if (int st = check_query(s, {who, q->flags, CTR_SHADE_LINEAR | CTR_SHADE_EXACT_POW, broken, q->n_rays, "n_rays",
                               q->d_origin && q->d_dir, "null rays"}))
    return st;
  if (q->n_rays == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_origin, "d_origin"}, {q->d_dir, "d_dir"}, {q->d_color, "d_color"},
                           {q->d_t, "d_t"}, {q->d_object, "d_object"}, {q->d_normal, "d_normal"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  ShadeLaunch L{};
  fill_lit(L, s, q->flags, CTR_SHADE_EXACT_POW);
  L.frames = ctr_shade_frames(q->bounces, s->flat.any_bounce);
  L.frame_dwords = s->flat.need_cold ? 10u : 4u;
  L.n_rays = (uint32_t)q->n_rays;
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
    return lds_fail(who, "the walk stack of this scene's mesh trees and " + std::to_string(L.frames) + " recursion frames need",
                    ctr_shade_lds_bytes(L), CTR_SHADE_LDS_MAX, "fewer bounces or CTR_SHADE_LINEAR fit");
  if (int st = use_device(s)) return st;
  return launched(ctr_launch_shade(L, hip_stream), "radiance query kernel launch");
}

extern "C" int ctr_shade_points(ctr_scene *s, const ctr_point_query *q, void *hip_stream) {
  const std::string who = "ctr_shade_points: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  const char *broken = "";
  if (!q->d_color && !q->d_light_shadow) broken = "no output: one of d_color and d_light_shadow is required";
  else if (q->d_color && (!q->d_normal || !q->d_view)) broken = "d_color needs d_normal and d_view";
  else if (q->d_material && q->d_object) broken = "d_material and d_object exclude each other";
  if (int st = check_query(s, {who, q->flags, CTR_POINTS_LINEAR | CTR_POINTS_EXACT_POW, broken, q->n_points, "n_points",
                               q->d_point != nullptr, "null d_point"}))
    return st;
  const size_t n_mat = s->flat.mats.size();
  if (q->d_color && !q->d_material && !q->d_object && (q->material < 0 || (size_t)q->material >= n_mat))
    return fail(CTR_E_INVALID, who + "material " + std::to_string(q->material) + " outside [0, " + std::to_string(n_mat) + ")");
  if (q->n_points == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_point, "d_point"}, {q->d_normal, "d_normal"}, {q->d_view, "d_view"}, {q->d_material, "d_material"},
                           {q->d_object, "d_object"}, {q->d_color, "d_color"}, {q->d_light_shadow, "d_light_shadow"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  PointsLaunch L{};
  const DScene D = fill_lit(L, s, q->flags, CTR_POINTS_EXACT_POW);
  L.n_mat = D.n_mat;
  L.n_obj = D.n_obj;
  L.n_points = (uint32_t)q->n_points;
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
    return lds_fail(who, "the walk stack of this scene's mesh trees needs", ctr_points_lds_bytes(L), CTR_POINTS_LDS_MAX,
                    "CTR_POINTS_LINEAR needs none");
  if (!L.color && !L.light_shadow) return CTR_OK;  // a scene without lights: the rows of d_light_shadow are empty
  if (int st = use_device(s)) return st;
  return launched(ctr_launch_points(L, hip_stream), "surface shading kernel launch");
}

extern "C" int ctr_list_hits(ctr_scene *s, const ctr_hit_query *q, void *hip_stream) {
  const std::string who = "ctr_list_hits: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  const bool any_slot = q->d_t || q->d_object || q->d_prim || q->d_point || q->d_normal || q->d_uv;
  std::string broken;
  if (q->max_hits == 0 || q->max_hits > CTR_HITS_MAX)
    broken = "max_hits " + std::to_string(q->max_hits) + " outside [1, " + std::to_string(CTR_HITS_MAX) + "]";
  else if (!(q->step >= 0.0) || std::isinf(q->step)) broken = "step must be finite and not negative";
  else if (!any_slot && !q->d_count) broken = "no output: d_count or one of the per-slot outputs is required";
  if (int st = check_query(s, {who, q->flags, CTR_HITS_IGNORE_TRANSPARENT | CTR_HITS_LINEAR, broken, q->n_rays, "n_rays",
                               q->d_origin && q->d_dir, "null rays"}))
    return st;
  if (any_slot && q->n_rays * q->max_hits >= 0x80000000ull)
    return fail(CTR_E_INVALID, who + "n_rays * max_hits must be below 2^31 with a per-slot output (d_count alone has no such limit)");
  if (q->n_rays == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_origin, "d_origin"}, {q->d_dir, "d_dir"}, {q->d_min_t, "d_min_t"}, {q->d_max_t, "d_max_t"},
                           {q->d_count, "d_count"}, {q->d_t, "d_t"}, {q->d_object, "d_object"}, {q->d_prim, "d_prim"},
                           {q->d_point, "d_point"}, {q->d_normal, "d_normal"}, {q->d_uv, "d_uv"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  if (int st = use_device(s)) return st;
  HitsLaunch L{};
  L.scene = ray_scene(s, device_scene(s));
  L.n_rays = (uint32_t)q->n_rays;
  L.flags = q->flags;
  L.max_hits = q->max_hits;
  L.min_t = q->min_t;
  L.max_t = q->max_t;
  L.step = q->step;
  L.origin = q->d_origin;
  L.dir = q->d_dir;
  L.min_t_arr = q->d_min_t;
  L.max_t_arr = q->d_max_t;
  L.count = q->d_count;
  L.t = q->d_t;
  L.object = q->d_object;
  L.prim = q->d_prim;
  L.point = q->d_point;
  L.normal = q->d_normal;
  L.uv = q->d_uv;
  return launched(ctr_launch_hits(L, hip_stream), "hit list kernel launch");
}

extern "C" int ctr_nearest_points(ctr_scene *s, const ctr_nearest_query *q, void *hip_stream) {
  const std::string who = "ctr_nearest_points: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  const char *broken = "";
  if (!q->d_distance && !q->d_object && !q->d_prim && !q->d_nearest && !q->d_normal)
    broken = "no output: one of d_distance, d_object, d_prim, d_nearest and d_normal is required";
  else if (!q->d_max_dist && !(q->max_dist >= 0.0f)) broken = "max_dist must not be negative or NaN";
  if (int st = check_query(s, {who, q->flags, CTR_NEAREST_LINEAR | CTR_NEAREST_SKIP_PLANES, broken, q->n_points, "n_points",
                               q->d_point != nullptr, "null d_point"}))
    return st;
  if (int st = check_object(s, who, q->object)) return st;
  if (q->n_points == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_point, "d_point"}, {q->d_max_dist, "d_max_dist"}, {q->d_distance, "d_distance"}, {q->d_object, "d_object"},
                           {q->d_prim, "d_prim"}, {q->d_nearest, "d_nearest"}, {q->d_normal, "d_normal"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  if (int st = use_device(s)) return st;
  NearestLaunch L{};
  L.scene = ray_scene(s, device_scene(s));
  L.n_points = (uint32_t)q->n_points;
  L.flags = q->flags;
  L.only = q->object;
  L.max_dist = q->max_dist;
  L.point = q->d_point;
  L.max_dist_arr = q->d_max_dist;
  L.distance = q->d_distance;
  L.object = q->d_object;
  L.prim = q->d_prim;
  L.nearest = q->d_nearest;
  L.normal = q->d_normal;
  return launched(ctr_launch_nearest(L, hip_stream), "nearest point kernel launch");
}

extern "C" int ctr_count_crossings(ctr_scene *s, const ctr_crossing_query *q, void *hip_stream) {
  const std::string who = "ctr_count_crossings: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  const char *broken = "";
  if (!q->d_count && !q->d_signed) broken = "no output: one of d_count and d_signed is required";
  if (int st = check_query(s, {who, q->flags, CTR_CROSS_LINEAR | CTR_CROSS_SKIP_PLANES | CTR_CROSS_SKIP_TRIANGLES, broken, q->n_rays, "n_rays",
                               q->d_origin && q->d_dir, "null rays"}))
    return st;
  if (int st = check_object(s, who, q->object)) return st;
  if (q->n_rays == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_origin, "d_origin"}, {q->d_dir, "d_dir"}, {q->d_min_t, "d_min_t"}, {q->d_max_t, "d_max_t"},
                           {q->d_count, "d_count"}, {q->d_signed, "d_signed"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  if (int st = use_device(s)) return st;
  CrossLaunch L{};
  L.scene = ray_scene(s, device_scene(s));
  L.n_rays = (uint32_t)q->n_rays;
  L.flags = q->flags;
  L.only = q->object;
  L.min_t = q->min_t;
  L.max_t = q->max_t;
  L.origin = q->d_origin;
  L.dir = q->d_dir;
  L.min_t_arr = q->d_min_t;
  L.max_t_arr = q->d_max_t;
  L.count = q->d_count;
  L.sgn = q->d_signed;
  return launched(ctr_launch_cross(L, hip_stream), "crossing count kernel launch");
}

extern "C" int ctr_inside_points(ctr_scene *s, const ctr_inside_query *q, void *hip_stream) {
  const std::string who = "ctr_inside_points: ";
  if (!q) return fail(CTR_E_INVALID, who + "null query");
  std::string broken;
  if (q->n_dirs > CTR_INSIDE_MAX_DIRS || (q->n_dirs && q->n_dirs % 2u == 0u))
    broken = "n_dirs " + std::to_string(q->n_dirs) + " is not 0 or an odd number up to " + std::to_string(CTR_INSIDE_MAX_DIRS);
  else if (q->n_dirs && !q->dirs) broken = "null dirs with n_dirs " + std::to_string(q->n_dirs);
  else if (!q->d_inside && !q->d_votes && !q->d_distance) broken = "no output: one of d_inside, d_votes and d_distance is required";
  InsideLaunch L{};
  if (broken.empty()) {
    L.n_dirs = q->n_dirs ? q->n_dirs : 3u;
    const float *dirs = q->n_dirs ? q->dirs : CROSS_DEFAULT_DIRS;
    for (uint32_t k = 0; k < L.n_dirs && broken.empty(); k++) {
      const float *d = dirs + 3 * k;
      if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]) || (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f))
        broken = "direction " + std::to_string(k) + " is not finite or is all zero";
      for (int c = 0; c < 3; c++) L.dirs[3 * k + c] = d[c];
    }
  }
  if (int st = check_query(s, {who, q->flags, CTR_INSIDE_LINEAR, broken, q->n_points, "n_points", q->d_point != nullptr, "null d_point"}))
    return st;
  if (int st = check_object(s, who, q->object)) return st;
  if (q->object >= 0) {
    const uint32_t type = s->flat.objs[(size_t)q->object].type;
    if (type != CTR_OBJ_MESH && type != CTR_OBJ_SPHERE)
      return fail(CTR_E_INVALID, who + "object " + std::to_string(q->object) + " is a " + (type == CTR_OBJ_PLANE ? "plane" : "stand-alone triangle") +
                                     ": only a mesh or a sphere bounds anything");
  }
  if (q->n_points == 0) return CTR_OK;
  const NamedPtr ptrs[] = {{q->d_point, "d_point"}, {q->d_inside, "d_inside"}, {q->d_votes, "d_votes"}, {q->d_distance, "d_distance"}};
  if (int st = check_device_pointers(s->device, who, ptrs)) return st;
  if (int st = use_device(s)) return st;
  L.scene = ray_scene(s, device_scene(s));
  L.n_points = (uint32_t)q->n_points;
  L.flags = q->flags;
  L.only = q->object;
  L.point = q->d_point;
  L.inside = q->d_inside;
  L.votes = q->d_votes;
  L.distance = q->d_distance;
  return launched(ctr_launch_inside(L, hip_stream), "inside kernel launch");
}

extern "C" void ctr_inside_default_dirs(float out[9]) {
  for (int k = 0; k < 9; k++) out[k] = CROSS_DEFAULT_DIRS[k];
}
