// query_check.cpp — the host glue of the ray queries that needs no device, as a program of its own (meant for ASan/UBSan; the
// record of a run: profiles/query_path/sanitizers.txt): the pointer classifier of ctr_scene.cpp and what is written on top of it
// (memory_kind, is_pinned, all_pinned, check_device_pointers), launched(), walk_stack_bytes and the two *_lds_bytes rules of
// ray_query.h / ray_shade.hip / ray_points.hip, and the checks ctr_cast_rays, ctr_shade_rays, ctr_shade_points, ctr_list_hits,
// ctr_nearest_points, ctr_count_crossings and ctr_inside_points make before they look at the scene.  Without a device the runtime knows no pointer: everything is HOST_OTHER, which is the path that
// swallows the runtime's error.  Linked with ctr_scene.cpp, ctr_rays.cpp, the query .hip files (ray_query, ray_shade, ray_points,
// ray_hits, ray_nearest and ray_cross since ctr_rays.cpp holds ctr_list_hits, ctr_nearest_points, ctr_count_crossings and
// ctr_inside_points: their host halves are what is checked; no check gets as far as a launch) and the host files those need:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -pthread -Wno-unused-function -Icutrace_amd/csrc -Iinclude
//     -o query_check scripts/query_check.cpp cutrace_amd/csrc/{ctr_scene.cpp,ctr_rays.cpp,ray_query.hip,ray_shade.hip,ray_points.hip,
//     ray_hits.hip,ray_nearest.hip,ray_cross.hip,guard_scan.hip,scene_flatten.cpp,guard.cpp,bvh.cpp}
//
//   query_check        prints "query_check: ok" and returns 0, or says what differed and returns 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctr_internal.h"
#include "cutrace_hits.h"
#include "cutrace_inside.h"
#include "cutrace_nearest.h"
#include "cutrace_rays.h"
#include "ray_points.h"
#include "ray_query.h"
#include "ray_shade.h"

static int failures = 0;
static void expect(bool ok, const char *what) {
  if (!ok) { fprintf(stderr, "query_check: %s\n", what); failures++; }
}
static void expect_error(int st, const char *text) {
  if (st != CTR_E_INVALID || strcmp(ctr_last_error(), text) != 0) {
    fprintf(stderr, "query_check: status %d \"%s\", expected %d \"%s\"\n", st, ctr_last_error(), CTR_E_INVALID, text);
    failures++;
  }
}

int main() {
  // ---- the classifier on memory the runtime does not know ----
  std::vector<float> heap(64);
  float stack[8] = {0};
  static float fixed[8];
  for (const void *p : {(const void *)heap.data(), (const void *)(heap.data() + 63), (const void *)stack, (const void *)fixed, (const void *)nullptr}) {
    expect(memory_kind(p).kind == MemKind::HOST_OTHER, "memory_kind: not HOST_OTHER");
    expect(!is_pinned(p), "is_pinned: true for pageable memory");
  }
  const HostFrame frame{heap.data(), heap.data() + 8, heap.data() + 32, nullptr};
  expect(!all_pinned(frame, 8) && !all_pinned(frame, 0) && !all_pinned(HostFrame{}, 8), "all_pinned");

  const NamedPtr none[] = {{nullptr, "d_a"}, {nullptr, "d_b"}};
  expect(check_device_pointers(0, "who: ", none) == CTR_OK, "check_device_pointers: null pointers are skipped");
  expect(check_device_pointers(0, "who: ", none, 0) == CTR_OK, "check_device_pointers: empty table");
  const NamedPtr some[] = {{nullptr, "d_a"}, {heap.data(), "d_b"}, {stack, "d_c"}};
  expect_error(check_device_pointers(0, "who: ", some), "who: d_b is not device memory of the scene's device");
  expect_error(check_device_pointers(3, "who: ", some + 2, 1, "device 3"), "who: d_c is not device memory of device 3");

  expect(launched(0, "a launch") == CTR_OK, "launched(0)");
  expect(launched((int)hipErrorInvalidValue, "a launch") == CTR_E_HIP_BASE + (int)hipErrorInvalidValue &&
             strncmp(ctr_last_error(), "a launch: hipErrorInvalidValue (", 32) == 0, "launched(hipErrorInvalidValue)");

  // ---- the walk stack and the LDS of a workgroup ----
  static_assert(walk_stack_bytes(0, 128, false) == 0 && walk_stack_bytes(24, 128, true) == 0, "no stack");
  static_assert(walk_stack_bytes(24, 128, false) == 24 * 128 * 4 && walk_stack_bytes(24, 64, false) == 24 * 64 * 4, "slots x lanes x 4");
  static_assert(walk_stack_bytes(0xFFFFFFFFu, 128, false) == (size_t)0xFFFFFFFFu * 512, "64-bit product");
  ShadeLaunch S{};
  S.scene.stack_slots = 24; S.frames = 15; S.frame_dwords = 10;
  expect(ctr_shade_lds_bytes(S) == (24 + 150) * 64 * 4, "ctr_shade_lds_bytes");
  S.flags = CTR_SHADE_LINEAR;
  expect(ctr_shade_lds_bytes(S) == 150 * 64 * 4, "ctr_shade_lds_bytes, linear");
  PointsLaunch P{};
  P.scene.stack_slots = 24;
  expect(ctr_points_lds_bytes(P) == 24 * 128 * 4, "ctr_points_lds_bytes");
  P.flags = CTR_POINTS_LINEAR | CTR_POINTS_EXACT_POW;
  expect(ctr_points_lds_bytes(P) == 0, "ctr_points_lds_bytes, linear");

  // ---- the three entry points up to the scene (tests/test_query_checks_cpu.py has every case; here: each path once) ----
  float *const some_ptr = heap.data();
  expect_error(ctr_cast_rays(nullptr, nullptr, nullptr), "ctr_cast_rays: null query");
  expect_error(ctr_shade_rays(nullptr, nullptr, nullptr), "ctr_shade_rays: null query");
  expect_error(ctr_shade_points(nullptr, nullptr, nullptr), "ctr_shade_points: null query");
  ctr_ray_query r{};
  r.n_rays = 2; r.d_origin = some_ptr; r.d_dir = some_ptr; r.d_t = some_ptr;
  expect_error(ctr_cast_rays(nullptr, &r, nullptr), "ctr_cast_rays: null scene");
  r.flags = 8;
  expect_error(ctr_cast_rays(nullptr, &r, nullptr), "ctr_cast_rays: unknown flag bits 8");
  r.flags = CTR_RAY_SHADOW;
  expect_error(ctr_cast_rays(nullptr, &r, nullptr), "ctr_cast_rays: CTR_RAY_SHADOW writes d_shadow only, and needs it");
  ctr_shade_query s{};
  s.n_rays = 2; s.d_origin = some_ptr; s.d_dir = some_ptr; s.d_color = some_ptr;
  expect_error(ctr_shade_rays(nullptr, &s, nullptr), "ctr_shade_rays: null scene");
  s.bounces = 16;
  expect_error(ctr_shade_rays(nullptr, &s, nullptr), "ctr_shade_rays: bounces 16 outside [0, 15]");
  ctr_point_query p{};
  p.n_points = 2; p.d_point = some_ptr; p.d_light_shadow = some_ptr;
  expect_error(ctr_shade_points(nullptr, &p, nullptr), "ctr_shade_points: null scene");
  p.d_color = some_ptr;
  expect_error(ctr_shade_points(nullptr, &p, nullptr), "ctr_shade_points: d_color needs d_normal and d_view");
  expect_error(ctr_list_hits(nullptr, nullptr, nullptr), "ctr_list_hits: null query");
  ctr_hit_query h{};
  h.n_rays = 2; h.max_hits = 4; h.step = 1e-3; h.d_count = (int32_t *)some_ptr;
  expect_error(ctr_list_hits(nullptr, &h, nullptr), "ctr_list_hits: null scene");
  h.max_hits = CTR_HITS_MAX + 1;
  expect_error(ctr_list_hits(nullptr, &h, nullptr), "ctr_list_hits: max_hits 65536 outside [1, 65535]");
  h.max_hits = 4; h.step = -1.0;
  expect_error(ctr_list_hits(nullptr, &h, nullptr), "ctr_list_hits: step must be finite and not negative");
  h.step = 0.0; h.d_count = nullptr;
  expect_error(ctr_list_hits(nullptr, &h, nullptr), "ctr_list_hits: no output: d_count or one of the per-slot outputs is required");
  expect_error(ctr_nearest_points(nullptr, nullptr, nullptr), "ctr_nearest_points: null query");
  ctr_nearest_query n{};
  n.n_points = 2; n.object = -1; n.d_point = some_ptr; n.d_distance = some_ptr;
  expect_error(ctr_nearest_points(nullptr, &n, nullptr), "ctr_nearest_points: null scene");
  n.max_dist = -1.0f;
  expect_error(ctr_nearest_points(nullptr, &n, nullptr), "ctr_nearest_points: max_dist must not be negative or NaN");
  n.max_dist = 1.0f; n.flags = 4;
  expect_error(ctr_nearest_points(nullptr, &n, nullptr), "ctr_nearest_points: unknown flag bits 4");
  n.flags = CTR_NEAREST_LINEAR | CTR_NEAREST_SKIP_PLANES; n.d_distance = nullptr;
  expect_error(ctr_nearest_points(nullptr, &n, nullptr), "ctr_nearest_points: no output: one of d_distance, d_object, d_prim, d_nearest and d_normal is required");

  // ---- the inside queries (include/cutrace_inside.h) ----
  expect_error(ctr_count_crossings(nullptr, nullptr, nullptr), "ctr_count_crossings: null query");
  ctr_crossing_query c{};
  c.n_rays = 2; c.object = -1; c.max_t = 1.0f; c.d_origin = some_ptr; c.d_dir = some_ptr; c.d_count = (int32_t *)some_ptr;
  expect_error(ctr_count_crossings(nullptr, &c, nullptr), "ctr_count_crossings: null scene");
  c.flags = 8 | CTR_CROSS_LINEAR;
  expect_error(ctr_count_crossings(nullptr, &c, nullptr), "ctr_count_crossings: unknown flag bits 8");
  c.flags = CTR_CROSS_LINEAR | CTR_CROSS_SKIP_PLANES | CTR_CROSS_SKIP_TRIANGLES; c.d_count = nullptr;
  expect_error(ctr_count_crossings(nullptr, &c, nullptr), "ctr_count_crossings: no output: one of d_count and d_signed is required");
  c.d_signed = (int32_t *)some_ptr;
  expect_error(ctr_count_crossings(nullptr, &c, nullptr), "ctr_count_crossings: null scene");
  expect_error(ctr_inside_points(nullptr, nullptr, nullptr), "ctr_inside_points: null query");
  ctr_inside_query in{};
  in.n_points = 2; in.object = -1; in.d_point = some_ptr; in.d_inside = (uint8_t *)some_ptr;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: null scene");
  in.flags = 2;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: unknown flag bits 2");
  in.flags = CTR_INSIDE_LINEAR; in.n_dirs = 2;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: n_dirs 2 is not 0 or an odd number up to 15");
  in.n_dirs = 17;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: n_dirs 17 is not 0 or an odd number up to 15");
  in.n_dirs = 15;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: null dirs with n_dirs 15");
  std::vector<float> table(45, 0.5f);   // exactly 15 directions: the copy reads all of them and nothing behind
  in.dirs = table.data();
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: null scene");
  table[42] = table[43] = table[44] = 0.0f;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: direction 14 is not finite or is all zero");
  table[3] = 1.0f / 0.0f;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: direction 1 is not finite or is all zero");
  in.n_dirs = 1; in.d_inside = nullptr;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: no output: one of d_inside, d_votes and d_distance is required");
  in.d_distance = some_ptr;
  expect_error(ctr_inside_points(nullptr, &in, nullptr), "ctr_inside_points: null scene");
  float def[9];
  ctr_inside_default_dirs(def);
  expect(def[0] == 0.3713907f && def[4] == 0.7462025f && def[8] == -0.5345225f, "ctr_inside_default_dirs");
  for (int k = 0; k < 9; k++) expect(def[k] != 0.0f, "a default direction with a zero component");

  if (!failures) printf("query_check: ok\n");
  return failures ? 1 : 0;
}
