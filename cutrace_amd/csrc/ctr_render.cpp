// ctr_render.cpp — the render path of include/cutrace_amd.h, cutrace_aa.h, cutrace_lens.h and cutrace_images.h on top of the scene
// handle (ctr_scene.cpp): every extern "C" render entry point checks its arguments, fills one RenderCall and hands it to
// render_device (the caller's device buffers and stream) or render_host (the caller's host buffers, the null stream).
//
// Replaces the host half of the reference's hot path:
//   gpu::render<S,bounces,tpb>   inc/kernel.hpp:86-130       → ctr_render / ctr_render_device
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "ctr_internal.h"
#include "cutrace_aa.h"
#include "cutrace_images.h"
#include "cutrace_lens.h"
#include "frame_images.h"
#include "kernel_choice.h"
#include "row_parts.h"
#include "tile_order.h"
#include "tile_shape.h"

#ifndef CTR_OCC6_MIN_TRIS
#define CTR_OCC6_MIN_TRIS 1000  // scenes with at least this many mesh triangles use the 6-waves-per-SIMD build
#endif

uint64_t ctr_scene::occ6_min_tris() {
  static const uint64_t v = [] { const char *e = getenv("CUTRACE_OCC6_MIN_TRIS"); return e ? (uint64_t)atoll(e) : (uint64_t)CTR_OCC6_MIN_TRIS; }();
  return v;
}

namespace {

// the caller's byte planes of ctr_render_images (null: not asked for)
struct HostImages { uint8_t *depth8, *color8, *normal8; };

// One render call as its entry point describes it, after the entry point's own checks.
struct RenderCall {
  float fudge;
  int bounces;
  const ctr_rows *rows;
  uint32_t first_frame = 0, n_frames = 1;  // the batch (device form only)
  uint64_t frame_stride_px = 0;
  uint32_t part_stride = 0;
  uint32_t ss_log2 = 0;            // != 0: one supersampled frame (rows, pixel counts and the buffers are the output's)
  const ctr_lens *lens = nullptr;  // the primary rays are the caller's, with ss_log2 one per sample (device form only)
  void *stream = nullptr;          // device form; the host form works on the null stream
  // device form: the caller's device buffers
  void *d_depth = nullptr, *d_color3 = nullptr, *d_normal3 = nullptr, *d_counters = nullptr;
  // host form: the caller's float buffers, or (images) its byte planes: chosen for as a render into pageable memory, `out` empty
  HostFrame out{};
  const HostImages *images = nullptr;
  ctr_render_stats *stats = nullptr;
  bool count = false;              // the counting launch of ctr_algorithmic_bytes
  unsigned long long *aabb_tris = nullptr;
};

// ---- the checks the entry points share; nothing here touches the GPU ----
int check_args(const ctr_scene *s, int bounces) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  if (bounces < 0 || bounces > CTR_MAX_BOUNCES)
    return fail(CTR_E_INVALID, "bounces must be in [0," + std::to_string(CTR_MAX_BOUNCES) + "]");
  if (s->cam.w == 0 || s->cam.h == 0) return fail(CTR_E_INVALID, "camera has zero width or height");
  return CTR_OK;
}

int check_outputs(const std::string &who, const RenderCall &c) {
  if (!c.d_depth || !c.d_color3 || !c.d_normal3) return fail(CTR_E_INVALID, who + "null output buffer");
  return CTR_OK;
}

// `samples` per axis as log2
int check_samples(const std::string &who, uint32_t samples, uint32_t &ls) {
  if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
    return fail(CTR_E_INVALID, who + "samples must be 1, 2, 4 or 8 per axis, got " + std::to_string(samples));
  ls = samples == 8 ? 3u : samples == 4 ? 2u : samples == 2 ? 1u : 0u;
  return CTR_OK;
}

// ---- the geometry of a launch: plain functions of the frame and the caller's rows; CTR_OK, or CTR_E_INVALID and the message in `err` ----
int make_rows(uint32_t frame_h, const ctr_rows *rin, DRows &R, std::string &err) {
  const uint64_t h = frame_h;
  ctr_rows r{0, h, h ? h : 1, 0, 1};
  if (rin && rin->row_end > rin->row_begin) {
    r = *rin;
    if (r.block_rows == 0) r.block_rows = h ? h : 1;
    if (r.n_parts == 0) { r.n_parts = 1; r.part = 0; }
    if (r.row_end > h) r.row_end = h;
  }
  const char *bad = r.part >= r.n_parts ? "ctr_rows: part >= n_parts" : nullptr;
  if (!bad && r.n_parts > 1 && (r.row_begin % r.block_rows) != 0) bad = "ctr_rows: row_begin must be a multiple of block_rows when n_parts > 1";
  if (bad) { err = bad; return CTR_E_INVALID; }
  // (one part: n_parts == 1 and part == 0 by now, the rows as they are)
  const PartRows own = r.n_parts > 1 ? part_rows(r.row_begin, r.row_end, r.block_rows, r.part, r.n_parts)
                                     : PartRows{0, r.row_end > r.row_begin ? r.row_end - r.row_begin : 0};
  R = DRows{(uint32_t)r.row_begin, (uint32_t)r.row_end, 0, (uint32_t)own.n_rows, (uint32_t)r.block_rows, r.part, r.n_parts, (uint32_t)own.first_block};
  return CTR_OK;
}

// make_rows, and for a batch whose parts rotate (part_stride) the per-frame tile grid sized for the largest part
int launch_rows(uint32_t frame_h, const ctr_rows *rin, uint32_t part_stride, DRows &R, std::string &err) {
  int st = make_rows(frame_h, rin, R, err);
  if (st || !part_stride || R.n_parts <= 1) return st;
  R.part_stride = part_stride % R.n_parts;
  uint32_t cap = 0;
  for (uint32_t p = 0; p < R.n_parts; p++) {
    ctr_rows rp = *rin;
    rp.part = p;
    DRows tmp{};
    if ((st = make_rows(frame_h, &rp, tmp, err))) return st;
    cap = tmp.n_rows > cap ? tmp.n_rows : cap;
  }
  R.n_rows = cap;
  return CTR_OK;
}

// The launch of the w x h output pixels becomes the launch of the s*w x s*h samples (one frame).  The part rule
// ((y / block_rows) % n_parts) == part is invariant under the scaling; first_block counts blocks and stays.
int aa_scale(uint32_t &w, uint32_t &h, DRows &R, uint32_t ls, std::string &err) {
  if (R.block_rows > h) R.block_rows = h;  // (rows end at h: a taller block selects what a block of h rows selects)
  w <<= ls; h <<= ls;
  R.row_begin <<= ls; R.row_end <<= ls; R.n_rows <<= ls; R.block_rows <<= ls;
  if ((uint64_t)tiles_x(w) * tiles_y(R.n_rows) <= 0x7FFFFFFFull) return CTR_OK;
  err = "supersampling: the sample frame has more than 0x7FFFFFFF tiles";
  return CTR_E_INVALID;
}

bool big_mesh(const ctr_scene *s) { return s->flat.mesh_tris >= ctr_scene::occ6_min_tris(); }

// What choose_kernel (kernel_choice.h) is told about this handle, the entry point and the call.
KernelFacts kernel_facts(const ctr_scene *s, KernelEntry entry, int bounces, bool deliverable) {
  const FlatScene &F = s->flat;
  return {s->user_variant, F.all_opaque, big_mesh(s), F.merged.built && F.merged.usable, entry, deliverable,
          stack_shape(bounces, F.any_bounce, F.need_cold), F.fast_pow_ok};
}

// ---- supersampling (include/cutrace_aa.h) ----
// The checks of the supersampling entry points after their own, in the order the header lists them: the scene and bounces, the
// samples rule, a build for the handle's variant bits, the size limits of the sample frame.  c.ss_log2 = log2 of `samples`.
int aa_precheck(const ctr_scene *s, KernelEntry entry, uint32_t samples, RenderCall &c) {
  uint32_t &ls = c.ss_log2;
  int st = check_args(s, c.bounces);
  if (st || (st = check_samples("", samples, ls)) || !ls) return st;
  if (choose_kernel(kernel_facts(s, entry, 0, false)).reject == KR_SS)
    return fail(CTR_E_INVALID, "supersampling: no build for CTR_VAR_STATS, CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER or CTR_VAR_NO_CLUSTER");
  if (((uint64_t)s->cam.w << ls) > 0xFFFFFFFFull || ((uint64_t)s->cam.h << ls) > 0xFFFFFFFFull)
    return fail(CTR_E_INVALID, "supersampling: samples x width or samples x height exceeds 32 bits");
  uint32_t w = s->cam.w, h = s->cam.h;
  DRows R{};
  std::string err;
  if ((st = make_rows(h, c.rows, R, err)) || (st = aa_scale(w, h, R, ls, err))) return fail(st, err);
  return CTR_OK;
}

// ---- the launch ----
// everything of the launch that the handle and the call fix before the rows and the build are known
void fill_launch(const ctr_scene *s, const RenderCall &c, RenderLaunch &L) {
  L.scene = device_scene(s);  // (tlas_root: set_root_and_head, once the launch's build is known, may put the merged tree there)
  L.cams = s->d_cams.as<DCam>();
  L.shards = s->d_shards.as<unsigned long long>();
  L.w = s->cam.w;
  L.h = s->cam.h;
  L.first_frame = c.first_frame;
  L.n_frames = c.n_frames;
  L.frame_stride_px = c.frame_stride_px;
  L.fudge = c.fudge;
  L.bounces = c.bounces;
  L.ss_log2 = c.ss_log2;
}

// The launch's top-level root and scene head.  A build that walks the merged tree (scene_flatten.h Merged) starts at the merged
// pseudo mesh; the top-level tree over the meshes stays the fallback the kernel itself takes for a cast the merged walk
// cannot decide (render_kernel.hip "merged walk").
void set_root_and_head(const ctr_scene *s, RenderLaunch &L, bool merged) {
  if (merged) L.scene.tlas_root = BVH_LEAF_FLAG | s->flat.n_mesh;
  // the scene head of THIS launch (scene_device.h DSceneHead), from the host copy the device arrays mirror: made here, per
  // launch, because the top-level root is final only now, and so that no edit of the arrays (guard selection, merged
  // tree, cameras) can leave a stale one behind
  if (!s->no_scene_head) fill_scene_head(s->flat, L.scene.tlas_root, L.head);
  L.no_shape = s->no_shape_build ? 1u : 0u;
  L.no_opaque = s->no_opaque_build ? 1u : 0u;
  L.no_phase_split = s->no_phase_split ? 1u : 0u;
  // the room facts only where the launch's kernel reads them (render_kernel.hip "room-safe lanes"): the one-mesh shape of the
  // any-hit builds, which then runs with the code that uses them, and the any-hit statistics builds; zero for every other launch
  if ((L.variant & KV_ANYHIT) && (ctr_launch_shape(L) == KS_ONE_MESH || (L.variant & KV_STATS))) fill_room_facts(s->flat, L.head, s->no_wall_skip);
  // ... and the dark-skip word where the kernel reads it ("dark lights"): the opaque one-mesh builds, which leave the casts out,
  // and the any-hit statistics builds, which count them
  if ((L.variant & KV_ANYHIT) && (ctr_launch_opaque(L) == KO_OPAQUE || (L.variant & KV_STATS))) fill_dark_skip(s->flat, L.head, s->no_dark_skip);
}

// the launch's room facts as the handle keeps them for ctr_debug_room_facts (written under the handle's mutex, like last_kernel)
ctr_scene::RoomWords room_words(const RenderLaunch &L) {
  return {{L.head.room_c[0], L.head.room_c[1], L.head.room_c[2]}, L.head.room_r, L.head.room_delta, L.head.room_lights};
}

// What the launch writes on the device: `spx` pixels per output buffer in the handle's `out`; for a direct launch (z: the
// caller's buffers as the device sees them, else null) also the groups' completion counters.
int prepare_outputs(ctr_scene *s, RenderLaunch &L, size_t spx, const HostFrame *z) {
  if (int st = s->h_counters.reserve(16)) return st;
  if (int st = s->out.reserve(spx)) return st;
  L.depth = s->out.as<float>();
  L.color = L.depth + spx;
  L.normal = L.depth + 4 * spx;
  if (!z) return CTR_OK;
  const size_t groups = (size_t)ctr_staging_groups(L);
  if (int st = reserve_both(s->d_groups, s->h_groups, groups)) return st;
  // cleared at the head of EVERY direct launch (a few microseconds): whatever an earlier launch left behind — one
  // that faulted or was cut short included — this one starts from zero
  HIP_TRY(hipMemsetAsync(s->d_groups.p, 0, groups * sizeof(uint32_t), nullptr));
  L.host_depth = z->depth;
  L.host_color = z->color3;
  L.host_normal = z->normal3;
  L.group_done = s->d_groups.as<uint32_t>();
  return CTR_OK;
}

// One device-to-host copy behind the kernel on the null stream (null dst: none): a direct DMA, queued, where the destination
// is page-locked from its first byte to its last (ctr_frame_alloc, hipHostMalloc, hipHostRegister); the runtime's staged
// copy where it is pageable.
hipError_t d2h(void *dst, const void *src, size_t bytes) {
  if (!dst) return hipSuccess;
  if (is_pinned(dst) && is_pinned((const char *)dst + bytes - 1)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, nullptr);
  return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}

// Copy-out (the reference does 3·h row-wise copies, kernel.hpp:110-114): ONE transfer when the three buffers are the
// consecutive parts of one page-locked block, else one per buffer (d2h).
int copy_out(ctr_scene *s, const RenderLaunch &L, const HostFrame &o, size_t px) {
  const bool packed = o.depth && o.color3 == o.depth + px && o.normal3 == o.color3 + 3 * px;
  if (packed && is_pinned(o.depth) && is_pinned(o.normal3 + 3 * px - 1)) {
    HIP_TRY(hipMemcpyAsync(o.depth, L.depth, sizeof(float) * 7 * px, hipMemcpyDeviceToHost, nullptr));
  } else {
    HIP_TRY(d2h(o.depth, L.depth, sizeof(float) * px));
    HIP_TRY(d2h(o.color3, L.color, sizeof(float) * 3 * px));
    HIP_TRY(d2h(o.normal3, L.normal, sizeof(float) * 3 * px));
  }
  if (o.uv2) HIP_TRY(hipMemcpy(o.uv2, s->uv.p, sizeof(float) * 2 * px, hipMemcpyDeviceToHost));
  return CTR_OK;
}

// ---- display frames (include/cutrace_images.h) ----
// In place of copy_out: the frame the launch left on the device is quantised behind it on the same stream, with the largest depth
// the launch itself accumulated in d_counters, and only the byte planes asked for leave the device: one copy per plane (d2h).
int images_out(ctr_scene *s, const RenderLaunch &L, const HostImages &o, size_t px) {
  if (int st = s->img.reserve(px)) return st;
  uint8_t *const img = s->img.as<uint8_t>();
  ImagesLaunch Q{};
  Q.n = px;
  Q.counters = s->d_counters.as<unsigned long long>();
  if (o.depth8) { Q.depth = L.depth; Q.depth8 = img; }
  if (o.color8) { Q.color = L.color; Q.color8 = img + 3 * px; }
  if (o.normal8) { Q.normal = L.normal; Q.normal8 = img + 6 * px; }
  if (int st = launched(ctr_launch_images(Q, nullptr), "quantise kernel launch")) return st;
  HIP_TRY(d2h(o.depth8, Q.depth8, 3 * px));
  HIP_TRY(d2h(o.color8, Q.color8, 3 * px));
  HIP_TRY(d2h(o.normal8, Q.normal8, 3 * px));
  return CTR_OK;
}

// A direct launch is over and h_groups holds its counters: did the whole frame reach the caller's buffers?
int check_delivery(ctr_scene *s, const RenderLaunch &L, const HostFrame &o, size_t spx, size_t n_groups) {
  // every group of tiles must have counted all its tiles, or its pixels never left for the caller's buffers
  // (how many tiles a group has is the kernel's business — its tile shape is a build option: ctr_group_tile_count)
  const uint32_t *const h_groups = s->h_groups.as<uint32_t>();
  size_t missing = 0;
  for (size_t g = 0; g < n_groups; g++)
    if (h_groups[g] != ctr_group_tile_count(L, g)) missing++;
  if (missing) {
    s->order.valid = false;  // whatever order that launch ran in is not to be trusted
    return fail(CTR_E_DELIVERY, std::to_string(missing) + " of " + std::to_string(n_groups) +
                " tile groups were not delivered to the caller's buffers (incomplete launch); render again");
  }
  if (!getenv("CUTRACE_VERIFY_DELIVERY")) return CTR_OK;
  // Debug aid for the kernel's own delivery (render_kernel.hip "Host delivery" relies on write-through stores and
  // scoped loads instead of fences): the tile-major staging copy of the frame is still on the device — fetch it
  // and compare every pixel with what arrived in the caller's buffers.
  std::vector<float> stg(7 * spx);
  HIP_TRY(hipMemcpy(stg.data(), L.depth, sizeof(float) * 7 * spx, hipMemcpyDeviceToHost));
  const uint32_t w = s->cam.w;
  uint64_t bad = 0;
  for (uint32_t y = 0; y < L.rows.n_rows; y++)
    for (uint32_t x = 0; x < w; x++) {
      const size_t at = (size_t)y * w + x, sp = (size_t)ctr_staging_index(L, x, y);
      bool ok = memcmp(&o.depth[at], &stg[sp], 4) == 0;
      ok = ok && memcmp(&o.color3[3 * at], &stg[spx + 3 * sp], 12) == 0 && memcmp(&o.normal3[3 * at], &stg[4 * spx + 3 * sp], 12) == 0;
      bad += ok ? 0 : 1;
    }
  if (bad) return fail(CTR_E_INVALID, "CUTRACE_VERIFY_DELIVERY: " + std::to_string(bad) + " delivered pixels differ from the staged frame");
  return CTR_OK;
}

// What the launch counted and how long it took: kept for ctr_last_counters, printed by the statistics / timing builds,
// returned in the call's `stats` and `aabb_tris`.
int report(ctr_scene *s, const RenderLaunch &L, std::chrono::high_resolution_clock::time_point t0, const RenderCall &c) {
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  unsigned long long cnt[16];
  memcpy(cnt, s->h_counters.p, sizeof(cnt));
  memcpy(s->last_cnt, cnt, sizeof(cnt));
  if (s->user_variant & CTR_VAR_STATS)
    fprintf(stderr, "cutrace_amd stats: wave_casts=%llu nodes=%llu tri_prefilter=%llu tri_exact=%llu mesh_entries=%llu "
                    "active_lanes=%llu node_lanes=%llu prefilter_lanes=%llu exact_lanes=%llu lane_max_nodes=%llu "
                    "lane_max_tris=%llu kernel_ms=%.3f\n", cnt[4], cnt[5],
            cnt[6], cnt[7], cnt[8], cnt[9], cnt[10], cnt[11], cnt[12], cnt[13], cnt[14], ms);
  if (c.aabb_tris) *c.aabb_tris = cnt[2];
  if (cnt[13] && !(s->user_variant & CTR_VAR_STATS))  // CTR_TIMING diagnostic build: share of the waves' lifetime
    fprintf(stderr, "cutrace_amd timing (%% of wave cycles): cast_setup=%.1f planes=%.1f object_loop=%.1f tlas+aabb=%.1f "
                    "mesh_setup=%.1f bvh_nodes=%.1f leaves=%.1f cont_mode=%.1f cont_rest=%.1f | wave_total=%llu kernel_ms=%.3f\n",
            100.0 * cnt[4] / cnt[13], 100.0 * cnt[5] / cnt[13], 100.0 * cnt[6] / cnt[13], 100.0 * cnt[7] / cnt[13],
            100.0 * cnt[8] / cnt[13], 100.0 * cnt[9] / cnt[13], 100.0 * cnt[10] / cnt[13], 100.0 * cnt[11] / cnt[13],
            100.0 * cnt[12] / cnt[13], cnt[13], ms);
  auto t1 = std::chrono::high_resolution_clock::now();
  if (ctr_render_stats *stats = c.stats) {
    stats->kernel_ms = ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    stats->ray_count = cnt[0];
    stats->rows = L.rows.n_rows >> L.ss_log2;  // (output rows)
    stats->max_depth = depth_of_counter(cnt[1]);
    stats->reserved = 0;
  }
  return CTR_OK;
}

// The device form: the caller's device buffers, counters and stream; nothing is waited for.
int render_device(ctr_scene *s, const RenderCall &c) {
  int st = check_args(s, c.bounces);
  if (st || (st = check_outputs("", c))) return st;
  const KernelEntry entry = c.lens ? (c.ss_log2 ? KE_DEVICE_LENS_SS : KE_DEVICE_LENS) : (c.ss_log2 ? KE_DEVICE_SS : KE_DEVICE);
  const KernelChoice choice = choose_kernel(kernel_facts(s, entry, c.bounces, false));
  if (choice.reject == KR_IGNTR_DEVICE) return fail(CTR_E_INVALID, "CTR_VAR_IGNORE_TRANSPARENT: host-buffer calls only (ctr_render, ctr_render_uv)");
  if (c.n_frames == 0 || c.first_frame >= s->n_cams || c.n_frames > s->n_cams - c.first_frame)
    return fail(CTR_E_INVALID, "frame range exceeds the cameras set with ctr_scene_set_cameras");
  if ((st = use_device(s))) return st;
  RenderLaunch L{};
  fill_launch(s, c, L);
  std::string err;
  if ((st = launch_rows(L.h, c.rows, c.part_stride, L.rows, err))) return fail(st, err);
  if (c.n_frames > 1 && c.frame_stride_px < (uint64_t)L.rows.n_rows * s->cam.w)
    return fail(CTR_E_INVALID, "frame_stride_px smaller than one frame's rows");
  L.depth = (float *)c.d_depth;
  L.color = (float *)c.d_color3;
  L.normal = (float *)c.d_normal3;
  L.counters = (unsigned long long *)c.d_counters;
  L.variant = choice.kv;
  if (c.lens) {
    L.ray_origin = c.lens->d_origin;
    L.ray_dir = c.lens->d_dir;
    L.ray_ambient = c.lens->ambient;
  }
  if (c.ss_log2 && (st = aa_scale(L.w, L.h, L.rows, c.ss_log2, err))) return fail(st, err);
  set_root_and_head(s, L, choice.merged);
  {
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((st = attach_order(s, L, big_mesh(s), false))) return st;
    s->last_kernel = L.variant;
    s->last_shape = ctr_launch_shape(L);
    s->last_opaque = ctr_launch_opaque(L);
    s->last_phased = ctr_launch_phased(L);
    s->last_room = room_words(L);
    s->last_dark_skip = (L.head.mesh_dark & CTR_HEAD_DARK) ? 1u : 0u;
  }
  return launched(ctr_launch_render(L, c.stream), "render kernel launch");
}

// The host form: the frame lands in the caller's host buffers (or, images, byte planes) before the call returns.
int render_host(ctr_scene *s, const RenderCall &c) {
  auto t0 = std::chrono::high_resolution_clock::now();
  int st = check_args(s, c.bounces);
  if (st) return st;
  std::lock_guard<std::mutex> lk(s->mtx);
  HIP_TRY(hipSetDevice(s->device));
  RenderLaunch L{};
  fill_launch(s, c, L);
  std::string err;
  if ((st = make_rows(L.h, c.rows, L.rows, err))) return fail(st, err);
  const size_t px = (size_t)L.rows.n_rows * s->cam.w;
  HostFrame z{};
  if (c.ss_log2 && (st = aa_scale(L.w, L.h, L.rows, c.ss_log2, err))) return fail(st, err);
  // an empty selection launches nothing and has no fourth output: it is chosen for as a plain render
  KernelFacts facts = kernel_facts(s, c.count ? KE_COUNT : c.ss_log2 ? KE_HOST_SS : c.out.uv2 && px ? KE_UV : KE_HOST, c.bounces, !c.images);
  if (!px) facts.user &= ~CTR_VAR_IGNORE_TRANSPARENT;
  KernelChoice choice = choose_kernel(facts);
  // (the caller's buffers are looked at only where everything else allows delivery by the kernel)
  if (choice.direct && !device_visible(c.out, px, z)) {
    facts.deliverable = false;
    choice = choose_kernel(facts);
  }
  const bool direct = choice.direct;
  const size_t spx = direct ? (size_t)ctr_staging_pixels(L) : (px ? px : 1);  // pixels per output buffer on the device
  if ((st = prepare_outputs(s, L, spx, direct ? &z : nullptr))) return st;
  L.counters = s->d_counters.as<unsigned long long>();
  if (choice.reject == KR_UV_STATS) return fail(CTR_E_INVALID, "ctr_render_uv / CTR_VAR_IGNORE_TRANSPARENT: not with the counting / statistics variants");
  L.variant = s->last_kernel = choice.kv;
  if (L.variant & KV_UV) {
    if ((st = s->uv.reserve(px))) return st;
    L.uv = s->uv.as<float>();
  }
  set_root_and_head(s, L, choice.merged);
  s->last_shape = ctr_launch_shape(L);
  s->last_opaque = ctr_launch_opaque(L);
  s->last_phased = ctr_launch_phased(L);
  s->last_room = room_words(L);
  s->last_dark_skip = (L.head.mesh_dark & CTR_HEAD_DARK) ? 1u : 0u;
  if ((st = attach_order(s, L, big_mesh(s), c.count))) return st;
  HIP_TRY(hipMemsetAsync(s->d_counters.p, 0, 16 * sizeof(unsigned long long), nullptr));
  HIP_TRY(hipEventRecord(s->ev0, nullptr));
  if ((st = launched(ctr_launch_render(L, nullptr), "render kernel launch"))) return st;
  HIP_TRY(hipEventRecord(s->ev1, nullptr));
  if (px && !direct && (st = c.images ? images_out(s, L, *c.images, px) : copy_out(s, L, c.out, px))) return st;
  HIP_TRY(hipMemcpyAsync(s->h_counters.p, s->d_counters.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr));
  const size_t n_groups = direct ? (size_t)ctr_staging_groups(L) : 0;
  if (direct) HIP_TRY(hipMemcpyAsync(s->h_groups.p, s->d_groups.p, n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (direct && (st = check_delivery(s, L, c.out, spx, n_groups))) return st;
  return report(s, L, t0, c);
}

}  // namespace

extern "C" {

int ctr_render_device_batch(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, uint32_t first_frame,
                            uint32_t n_frames, uint64_t frame_stride_px, uint32_t part_stride, void *d_depth,
                            void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  return render_device(s, {.fudge = fudge, .bounces = bounces, .rows = rows, .first_frame = first_frame, .n_frames = n_frames,
                           .frame_stride_px = frame_stride_px, .part_stride = part_stride, .stream = hip_stream, .d_depth = d_depth,
                           .d_color3 = d_color3, .d_normal3 = d_normal3, .d_counters = d_counters});
}

int ctr_render_device(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, void *d_depth, void *d_color3,
                      void *d_normal3, void *d_counters, void *hip_stream) {
  return render_device(s, {.fudge = fudge, .bounces = bounces, .rows = rows, .stream = hip_stream, .d_depth = d_depth,
                           .d_color3 = d_color3, .d_normal3 = d_normal3, .d_counters = d_counters});
}

int ctr_render_device_aa(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, void *d_depth,
                         void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  RenderCall c{.fudge = fudge, .bounces = bounces, .rows = rows, .stream = hip_stream, .d_depth = d_depth,
               .d_color3 = d_color3, .d_normal3 = d_normal3, .d_counters = d_counters};
  if (int st = aa_precheck(s, KE_DEVICE_SS, samples, c)) return st;
  return render_device(s, c);
}

// include/cutrace_lens.h.  Every check comes before the GPU is touched (hipPointerGetAttributes asks the runtime, no device work)
int ctr_render_device_lens(ctr_scene *s, float fudge, int bounces, const ctr_lens *lens, const ctr_rows *rows, void *d_depth,
                           void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  const std::string who = "ctr_render_device_lens: ";
  RenderCall c{.fudge = fudge, .bounces = bounces, .rows = rows, .lens = lens, .stream = hip_stream, .d_depth = d_depth,
               .d_color3 = d_color3, .d_normal3 = d_normal3, .d_counters = d_counters};
  int st = check_args(s, bounces);
  if (st) return st;
  if (!lens) return fail(CTR_E_INVALID, who + "null lens");
  if (!lens->d_origin || !lens->d_dir) return fail(CTR_E_INVALID, who + "null rays");
  const uint32_t samples = lens->samples;
  uint32_t ls = 0;
  if ((st = check_outputs(who, c)) || (st = check_samples(who, samples, ls))) return st;
  if (choose_kernel(kernel_facts(s, ls ? KE_DEVICE_LENS_SS : KE_DEVICE_LENS, bounces, false)).reject == KR_LENS)
    return fail(CTR_E_INVALID, who + "no build for CTR_VAR_STATS, CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER or CTR_VAR_NO_CLUSTER");
  if ((st = aa_precheck(s, KE_DEVICE_SS, samples, c))) return st;  // (the size limits of the sample frame)
  // (w, h <= 2^32 / s each, s*s <= 64: the product fits 64 bits)
  const uint64_t want = ((uint64_t)s->cam.w << ls) * ((uint64_t)s->cam.h << ls);
  if (lens->n_rays != want)
    return fail(CTR_E_INVALID, who + "n_rays is " + std::to_string(lens->n_rays) + ", the " + std::to_string(samples) + " x " + std::to_string(samples) +
                                   " samples of the " + std::to_string(s->cam.w) + " x " + std::to_string(s->cam.h) + " frame are " + std::to_string(want));
  const NamedPtr ptrs[] = {{lens->d_origin, "d_origin"}, {lens->d_dir, "d_dir"}};
  if ((st = check_device_pointers(s->device, who, ptrs))) return st;
  return render_device(s, c);
}

int ctr_render(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, float *depth, float *color3,
               float *normal3, ctr_render_stats *stats) {
  return render_host(s, {.fudge = fudge, .bounces = bounces, .rows = rows, .out = {depth, color3, normal3, nullptr}, .stats = stats});
}

int ctr_render_uv(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, float *depth, float *color3,
                  float *normal3, float *uv2, ctr_render_stats *stats) {
  if (!uv2) return fail(CTR_E_INVALID, "ctr_render_uv: null uv buffer");
  return render_host(s, {.fudge = fudge, .bounces = bounces, .rows = rows, .out = {depth, color3, normal3, uv2}, .stats = stats});
}

int ctr_render_aa(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, float *depth, float *color3,
                  float *normal3, ctr_render_stats *stats) {
  RenderCall c{.fudge = fudge, .bounces = bounces, .rows = rows, .out = {depth, color3, normal3, nullptr}, .stats = stats};
  if (int st = aa_precheck(s, KE_HOST_SS, samples, c)) return st;
  return render_host(s, c);
}

// include/cutrace_images.h
int ctr_render_images(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, uint8_t *depth8,
                      uint8_t *color8, uint8_t *normal8, ctr_render_stats *stats) {
  if (!depth8 && !color8 && !normal8) return fail(CTR_E_INVALID, "ctr_render_images: no destination plane");
  const HostImages images{depth8, color8, normal8};
  RenderCall c{.fudge = fudge, .bounces = bounces, .rows = rows, .images = &images, .stats = stats};
  if (int st = aa_precheck(s, KE_HOST_SS, samples, c)) return st;
  return render_host(s, c);
}

int ctr_quantise_device(int device, const ctr_image_planes *p, void *hip_stream) {
  const std::string who = "ctr_quantise_device: ";
  if (!p) return fail(CTR_E_INVALID, who + "null planes");
  if (p->reserved) return fail(CTR_E_INVALID, who + "reserved must be 0");
  const NamedPtr ptrs[] = {{p->d_depth, "d_depth"}, {p->d_color3, "d_color3"}, {p->d_normal3, "d_normal3"}, {p->d_depth8, "d_depth8"},
                           {p->d_color8, "d_color8"}, {p->d_normal8, "d_normal8"}, {p->d_counters, "d_counters"}};
  for (int k = 0; k < 3; k++) {
    const NamedPtr &have = ptrs[k].p ? ptrs[k] : ptrs[3 + k], &lack = ptrs[k].p ? ptrs[3 + k] : ptrs[k];
    if (!have.p != !lack.p) return fail(CTR_E_INVALID, who + have.name + " without " + lack.name);
  }
  if (!p->d_depth && !p->d_color3 && !p->d_normal3) return fail(CTR_E_INVALID, who + "no plane");
  if (p->n_pixels == 0) return CTR_OK;
  if (int st = check_device_pointers(device, who, ptrs, ("device " + std::to_string(device)).c_str())) return st;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != device) HIP_TRY(hipSetDevice(device));
  const ImagesLaunch Q{p->n_pixels, p->d_depth, p->d_color3, p->d_normal3, p->d_depth8, p->d_color8, p->d_normal8,
                       (const unsigned long long *)p->d_counters, p->max_depth};
  return launched(ctr_launch_images(Q, hip_stream), "quantise kernel launch");
}

int ctr_algorithmic_bytes(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, uint64_t *bytes,
                          uint64_t *ray_count) {
  ctr_render_stats stt{};
  unsigned long long aabb = 0;
  int st = render_host(s, {.fudge = fudge, .bounces = bounces, .rows = rows, .stats = &stt, .count = true, .aabb_tris = &aabb});
  if (st) return st;
  // 56·N_obj per ray_cast + 48·N_tri per AABB-hit mesh + 28 B per pixel written
  if (bytes) *bytes = 56ull * s->flat.objs.size() * stt.ray_count + 48ull * aabb + 28ull * stt.rows * s->cam.w;
  if (ray_count) *ray_count = stt.ray_count;
  return CTR_OK;
}

}  // extern "C"
