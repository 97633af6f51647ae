// ctr_api.cpp — the C-ABI of include/cutrace_amd.h on top of the gfx950 kernel: handle lifetime, uploads, the
// launch set-up and the extern "C" entry points.
//
// Replaces the host half of the reference's hot path:
//   cpu_to_gpu::convert          inc/cpu_to_gpu.hpp:188-198  → ctr_scene_create (flatten_scene, scene_flatten.cpp, then one
//                                                               flat upload, hipMalloc + hipMemcpy, no managed memory)
//   gpu::render<S,bounces,tpb>   inc/kernel.hpp:86-130       → ctr_render / ctr_render_device
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "ctr_internal.h"
#include "cutrace_aa.h"
#include "cutrace_amd.h"
#include "cutrace_images.h"
#include "cutrace_lens.h"
#include "frame_images.h"
#include "guard.h"
#include "kernel_choice.h"
#include "row_parts.h"
#include "scene_device.h"
#include "scene_flatten.h"
#include "tile_order.h"

namespace {
thread_local std::string g_err;
}

// ---- what ctr_internal.h declares for every host translation unit ----
int fail(int code, const std::string &msg) {
  g_err = msg;
  fprintf(stderr, "cutrace_amd: %s\n", msg.c_str());  // print-and-continue, like cudaCheck (inc/cuda.hpp:12-22)
  return code;
}
int hip_fail(hipError_t e, const char *what) {
  return fail(CTR_E_HIP_BASE + (int)e, std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

bool is_pinned(const void *p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // plain malloc'ed memory: "invalid value", not an error of ours
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

bool device_view(float *host, float **dev) {
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess || !d) {
    (void)hipGetLastError();
    return false;
  }
  *dev = (float *)d;
  return true;
}

bool all_pinned(const HostFrame &o, size_t px) {
  return px && o.depth && o.color3 && o.normal3 &&
         is_pinned(o.depth) && is_pinned(o.depth + px - 1) && is_pinned(o.color3) && is_pinned(o.color3 + 3 * px - 1) &&
         is_pinned(o.normal3) && is_pinned(o.normal3 + 3 * px - 1);
}

// Page-locked destinations (ctr_frame_alloc, hipHostMalloc, mapped hipHostRegister) are visible to the device:
// the kernel then delivers the frame ITSELF, group of tiles by group of tiles while it renders (render_kernel.hip
// "Host delivery"), so the 28 bytes per pixel cross PCIe underneath the rendering instead of in a DMA after it.
// Any other destination: device buffers + copies (copy_out).
bool device_visible(const HostFrame &o, size_t px, HostFrame &z) {
  return all_pinned(o, px) && device_view(o.depth, &z.depth) && device_view(o.color3, &z.color3) &&
         device_view(o.normal3, &z.normal3);
}

int use_device(const ctr_scene *s) {
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != s->device) HIP_TRY(hipSetDevice(s->device));
  return CTR_OK;
}

void ctr_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }

#ifndef CTR_OCC6_MIN_TRIS
#define CTR_OCC6_MIN_TRIS 1000  // scenes with at least this many mesh triangles use the 6-waves-per-SIMD build
#endif
#ifndef CTR_FIRST_ORDER_MIN_TILES
#define CTR_FIRST_ORDER_MIN_TILES 8192  // smaller launches start in image order: one round of waves, no tail to shape
#endif
#ifndef CTR_ORDER_PERIOD
#define CTR_ORDER_PERIOD 8  // launches between rebuilds of the tile order
#endif

uint64_t ctr_scene::occ6_min_tris() {
  static const uint64_t v = [] { const char *e = getenv("CUTRACE_OCC6_MIN_TRIS"); return e ? (uint64_t)atoll(e) : (uint64_t)CTR_OCC6_MIN_TRIS; }();
  return v;
}

namespace {

DCam to_dcam(const ctr_camera &c) {
  DCam cam{};
  cam.pos[0] = c.pos.x; cam.pos[1] = c.pos.y; cam.pos[2] = c.pos.z;
  cam.up[0] = c.up.x; cam.up[1] = c.up.y; cam.up[2] = c.up.z;
  cam.forward[0] = c.forward.x; cam.forward[1] = c.forward.y; cam.forward[2] = c.forward.z;
  cam.right[0] = c.right.x; cam.right[1] = c.right.y; cam.right[2] = c.right.z;
  cam.ambient = c.ambient;
  cam.w = (uint32_t)c.w;
  cam.h = (uint32_t)c.h;
  return cam;
}

// The scene's ten device arrays, each ONCE: its pointer in the handle, its host copy (scene_flatten.h FlatScene), the bytes
// of the whole array and of one record, and the key under which a DirtyRange names it (-1: never edited after the
// upload).  ctr_scene_create uploads, upload_dirty re-uploads and ctr_scene_destroy frees by this table.
// F: s->flat, or what ctr_scene_create is about to move there.
struct SceneArray { void **dev; const void *host; size_t bytes, rec; int dirty; };
std::vector<SceneArray> scene_arrays(ctr_scene *s, const FlatScene &F) {
  auto row = [](auto &dev, const auto &v, int dirty = -1, size_t rec = 0) {
    return SceneArray{(void **)&dev, v.data(), v.size() * sizeof(v[0]), rec ? rec : sizeof(v[0]), dirty};
  };
  return {row(s->d_objs, F.objs, DirtyRange::OBJS), row(s->d_oloop, F.oloop), row(s->d_meshes, F.meshes, DirtyRange::MESHES),
          row(s->d_planes, F.planes), row(s->d_tris, F.tris, DirtyRange::TRIS), row(s->d_nodes, F.nodes),
          row(s->d_nodes4, F.nodes4, DirtyRange::NODES4), row(s->d_gnorm, F.gn, DirtyRange::GNORM, 4 * sizeof(float)),
          row(s->d_lights, F.lights), row(s->d_mats, F.mats)};
}

// Buffers that only grow: when `need` elements exceed `cap`, every buffer of the list is freed and allocated anew for
// `need` elements of its size (`host`: page-locked host memory).  An allocation that fails leaves cap == 0 — and, of
// the buffers, some null — so that the next call comes back here whatever its size.
struct GrowBuf { void **p; size_t elem; bool host; };
int grow(size_t need, size_t &cap, std::initializer_list<GrowBuf> bufs) {
  if (need <= cap) return CTR_OK;
  cap = 0;
  for (const GrowBuf &b : bufs) {
    if (*b.p) (void)(b.host ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
  }
  for (const GrowBuf &b : bufs) HIP_TRY(b.host ? hipHostMalloc(b.p, need * b.elem, hipHostMallocDefault) : hipMalloc(b.p, need * b.elem));
  cap = need;
  return CTR_OK;
}

int make_rows(const ctr_scene *s, const ctr_rows *rin, DRows &R) {
  const uint64_t h = s->cam.h;
  ctr_rows r{0, h, h ? h : 1, 0, 1};
  if (rin && rin->row_end > rin->row_begin) {
    r = *rin;
    if (r.block_rows == 0) r.block_rows = h ? h : 1;
    if (r.n_parts == 0) { r.n_parts = 1; r.part = 0; }
    if (r.row_end > h) r.row_end = h;
  }
  if (r.part >= r.n_parts) return fail(CTR_E_INVALID, "ctr_rows: part >= n_parts");
  if (r.n_parts > 1 && (r.row_begin % r.block_rows) != 0)
    return fail(CTR_E_INVALID, "ctr_rows: row_begin must be a multiple of block_rows when n_parts > 1");
  R.row_begin = (uint32_t)r.row_begin;
  R.row_end = (uint32_t)r.row_end;
  R.part_stride = 0;
  R.block_rows = (uint32_t)r.block_rows;
  R.part = r.part;
  R.n_parts = r.n_parts;
  if (r.n_parts <= 1) {
    R.n_rows = (uint32_t)(r.row_end > r.row_begin ? r.row_end - r.row_begin : 0);
    R.first_block = 0;
    R.n_parts = 1;
    R.part = 0;
  } else {
    const PartRows own = part_rows(r.row_begin, r.row_end, r.block_rows, r.part, r.n_parts);
    R.first_block = (uint32_t)own.first_block;
    R.n_rows = (uint32_t)own.n_rows;
  }
  return CTR_OK;
}

void fill_launch(const ctr_scene *s, RenderLaunch &L) {
  const FlatScene &F = s->flat;
  L.objs = s->d_objs;
  L.oloop = s->d_oloop;
  L.meshes = s->d_meshes;
  L.n_mesh = F.n_mesh;
  L.tlas_root = F.tlas_root;          // (set_root_and_head, once the launch's build is known, may put the merged tree here)
  L.tlas_root_regular = F.tlas_root;
  L.tlas_begin = F.tlas_begin;
  for (int q = 0; q < 3; q++) { L.tl_mn[q] = F.tl_mn[q]; L.tl_mx[q] = F.tl_mx[q]; }
  L.planes = s->d_planes;
  L.n_oloop = (uint32_t)F.oloop.size();
  L.n_plane_recs = (uint32_t)F.planes.size();
  L.n_axis_recs = F.n_axis_recs;
  L.tris = s->d_tris;
  L.nodes = s->d_nodes;
  L.nodes4 = s->d_nodes4;
  L.gnorm = s->d_gnorm;
  L.lights = s->d_lights;
  L.mats = s->d_mats;
  L.n_obj = (uint32_t)F.objs.size();
  L.n_light = (uint32_t)F.lights.size();
  L.n_mat = (uint32_t)F.mats.size();
  L.has_mesh = F.has_mesh ? 1u : 0u;
  L.need_cold_frames = F.need_cold ? 1u : 0u;
  L.any_bounce = F.any_bounce ? 1u : 0u;
  L.cams = s->d_cams;
  L.shards = s->d_shards;
  L.w = s->cam.w;
  L.h = s->cam.h;
  L.first_frame = 0;
  L.n_frames = 1;
  L.frame_stride_px = 0;
}

// What choose_kernel (kernel_choice.h) is told about this handle, the entry point and the call.
KernelFacts kernel_facts(const ctr_scene *s, KernelEntry entry, int bounces, bool deliverable) {
  const FlatScene &F = s->flat;
  return {s->user_variant, F.all_opaque, F.mesh_tris >= ctr_scene::occ6_min_tris(), F.merged.built && F.merged.usable, entry, deliverable,
          stack_shape(bounces, F.any_bounce, F.need_cold), F.fast_pow_ok};
}

// The launch's top-level root and scene head.  A build that walks the merged tree (scene_flatten.h Merged) starts at the merged
// pseudo mesh; the top-level tree over the meshes stays the fallback the kernel itself takes for a cast the merged walk
// cannot decide (render_kernel.hip "merged walk").
void set_root_and_head(const ctr_scene *s, RenderLaunch &L, bool merged) {
  if (merged) L.tlas_root = BVH_LEAF_FLAG | s->flat.n_mesh;
  // the scene head of THIS launch (scene_device.h DSceneHead), from the host copy the device arrays mirror: made here, per
  // launch, because the top-level root is final only now, and so that no edit of the arrays (guard selection, merged
  // tree, cameras) can leave a stale one behind
  if (!s->no_scene_head) fill_scene_head(s->flat, L.tlas_root, L.head);
}

// Attach the tile-order buffers to a launch: use the stored order when the launch has the shape the
// order was measured on, and have the launch record costs + sort them for the next one.
int attach_order(ctr_scene *s, RenderLaunch &L, bool count) {
  L.order = nullptr;
  L.cost = nullptr;
  L.order_next = nullptr;
  if ((s->user_variant & (CTR_VAR_NO_REORDER | CTR_VAR_STATS)) || count) return CTR_OK;
  const uint64_t n = ctr_launch_waves(L);
  if (n == 0 || n > 0x7FFFFFFFull) return CTR_OK;
  if (n > s->order_cap) s->order_valid = false;  // new buffers hold no order
  if (int st = grow(n, s->order_cap, {{(void **)&s->d_cost, sizeof(uint32_t), false}, {(void **)&s->d_order, sizeof(uint32_t), false}})) return st;
  const uint64_t key[6] = {n, ((uint64_t)L.w << 32) | L.h, ((uint64_t)L.rows.row_begin << 32) | L.rows.row_end,
                           ((uint64_t)L.rows.block_rows << 32) | L.rows.n_parts,
                           ((uint64_t)L.rows.part << 32) | L.rows.part_stride,
                           ((uint64_t)(L.group_done ? 1u : 0u) << 32) | L.n_frames};  // (host delivery orders tiles by group)
  const bool same = s->order_valid && memcmp(key, s->order_key, sizeof(key)) == 0;
  // (a shape's first launch runs in image order: an a-priori estimate — tiles whose primary rays meet the box
  //  of a mesh / sphere, computed and sorted by a pre-pass — was built and measured in round 2: the expensive
  //  tiles of these scenes are speckle along shadow edges and reflections, not the tiles that look at an
  //  object, and the pre-pass cost more than it won; DESIGN.md "First launch")
  if (same) L.order = s->d_order;
  else {
    s->order_age = 0;
    // a shape nothing is known about: centre-out instead of image order (tile_order.hip first_order) — for
    // launches large enough to have a tail and scenes heavy enough (the triangle count that also picks the 6-wave
    // build) for the ~8 us of the order kernel to pay: bunny -5.5 %, 64k bunny -2 %, C4 -2 %, but mirror.json (924
    // triangles, 0.2 ms) +4 % (profiles/r02/first_launch_centre_out.txt)
    if (n >= CTR_FIRST_ORDER_MIN_TILES && s->flat.mesh_tris >= ctr_scene::occ6_min_tris() && !(s->user_variant & CTR_VAR_IMAGE_ORDER_FIRST)) {
      L.order = s->d_order;
      L.order_init = 1;
    }
  }
  memcpy(s->order_key, key, sizeof(key));
  s->order_valid = true;  // after this launch d_order holds an order measured on this shape
  L.cost = s->d_cost;
  // The order is rebuilt after the first two launches of a shape (the second one measured under the
  // new order); after that every launch while the view keeps changing (a camera path: 90-frame
  // orbit 1.46 ms/frame rebuilt every frame vs 1.59 every 8th, 1.77 without scheduling), and only
  // every CTR_ORDER_PERIOD-th launch while the same view is rendered again and again.
  const uint64_t view = ((uint64_t)s->cams_epoch << 32) | L.first_frame;
  const bool same_view = same && view == s->order_view;
  s->order_view = view;
  if (s->order_age < 2 || !same_view || s->order_age % CTR_ORDER_PERIOD == 0) L.order_next = s->d_order;
  s->order_age++;
  if (s->poison_next_order) {
    // test hook: this launch gets an order whose second half names no tile — those waves leave at once, their tiles
    // are never rendered, and (host delivery) their groups never complete
    s->poison_next_order = false;
    std::vector<uint32_t> o(n);
    for (uint64_t k = 0; k < n; k++) o[k] = k < n / 2 ? (uint32_t)k : 0xFFFFFFFFu;
    HIP_TRY(hipMemcpy(s->d_order, o.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    L.order = s->d_order;
    L.order_init = 0;
    L.order_next = nullptr;
    s->order_valid = false;  // the next launch starts over
  }
  return CTR_OK;
}

// the device receives the records a host-side edit changed (scene_flatten.h DirtyRange), in the order of the list
int upload_dirty(ctr_scene *s, const std::vector<DirtyRange> &dirty) {
  const std::vector<SceneArray> arrays = scene_arrays(s, s->flat);
  for (const DirtyRange &r : dirty)
    for (const SceneArray &a : arrays) {
      if (a.dirty != (int)r.array || !r.count) continue;
      const void *src = r.payload.empty() ? (const char *)a.host + r.begin * a.rec : (const char *)r.payload.data();
      HIP_TRY(hipMemcpy((char *)*a.dev + r.begin * a.rec, src, r.count * a.rec, hipMemcpyHostToDevice));
    }
  return CTR_OK;
}

// The guard of the BVH culling (guard.cpp): at upload and whenever the cameras change — plan, apply to the host copy,
// upload what changed.
int refresh_linear_meshes(ctr_scene *s) {
  const GuardPlan plan = plan_guards(s->flat, s->h_cams);
  const std::vector<DirtyRange> dirty = apply_guards(s->flat, plan);
  if (getenv("CUTRACE_DEBUG_GUARDS")) {
    size_t per_mesh = 0;
    for (const MeshGuard &g : s->flat.guards) per_mesh += g.guarded.size();
    fprintf(stderr, "cutrace_amd guards: %zu origins (eyes + mirror images), %zu mirrors, %zu guard records over %zu meshes, merged keys %zu, linear %d\n",
            plan.n_origins, plan.n_mirrors, per_mesh, s->flat.guards.size(), plan.merged_keys.size(), (int)plan.any_linear);
  }
  return upload_dirty(s, dirty);
}

// The merged tree of a scene that has room for it (scene_flatten.h Merged): built, uploaded, guarded.
int build_merged_tree(ctr_scene *s) {
  const std::vector<DirtyRange> dirty = ::build_merged_tree(s->flat);
  if (dirty.empty()) return CTR_OK;
  if (int st = upload_dirty(s, dirty)) {
    s->flat.merged.built = false;  // (the device never got it: the next ctr_set_variant builds it again)
    return st;
  }
  return refresh_linear_meshes(s);
}

int check_args(const ctr_scene *s, int bounces) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  if (bounces < 0 || bounces > CTR_MAX_BOUNCES)
    return fail(CTR_E_INVALID, "bounces must be in [0," + std::to_string(CTR_MAX_BOUNCES) + "]");
  if (s->cam.w == 0 || s->cam.h == 0) return fail(CTR_E_INVALID, "camera has zero width or height");
  return CTR_OK;
}

// ---- supersampling (include/cutrace_aa.h) ----
// `samples` as log2, or why the handle cannot make the call; nothing here touches the GPU
int aa_check(const ctr_scene *s, KernelEntry entry, uint32_t samples, uint32_t &ls) {
  if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
    return fail(CTR_E_INVALID, "samples must be 1, 2, 4 or 8 per axis, got " + std::to_string(samples));
  ls = samples == 8 ? 3u : samples == 4 ? 2u : samples == 2 ? 1u : 0u;
  if (!ls) return CTR_OK;
  if (choose_kernel(kernel_facts(s, entry, 0, false)).reject == KR_SS)
    return fail(CTR_E_INVALID, "supersampling: no build for CTR_VAR_STATS, CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER or CTR_VAR_NO_CLUSTER");
  if (((uint64_t)s->cam.w << ls) > 0xFFFFFFFFull || ((uint64_t)s->cam.h << ls) > 0xFFFFFFFFull)
    return fail(CTR_E_INVALID, "supersampling: samples x width or samples x height exceeds 32 bits");
  return CTR_OK;
}
// The launch of the w x h output pixels (fill_launch, make_rows) becomes the launch of the s*w x s*h samples.  The part rule
// ((y / block_rows) % n_parts) == part is invariant under the scaling; first_block counts blocks and stays.
int aa_scale(RenderLaunch &L, uint32_t ls) {
  DRows &R = L.rows;
  if (R.block_rows > L.h) R.block_rows = L.h;  // (rows end at h: a taller block selects what a block of h rows selects)
  L.w <<= ls; L.h <<= ls;
  R.row_begin <<= ls; R.row_end <<= ls; R.n_rows <<= ls; R.block_rows <<= ls;
  L.ss_log2 = ls;
  if (ctr_launch_waves(L) > 0x7FFFFFFFull) return fail(CTR_E_INVALID, "supersampling: the sample frame has more than 0x7FFFFFFF tiles");
  return CTR_OK;
}
// the checks of both entry points, in the order the header lists them
int aa_precheck(ctr_scene *s, KernelEntry entry, int bounces, uint32_t samples, const ctr_rows *rows, uint32_t &ls) {
  int st = check_args(s, bounces);
  if (st || (st = aa_check(s, entry, samples, ls)) || !ls) return st;
  RenderLaunch L{};
  L.w = s->cam.w; L.h = s->cam.h; L.n_frames = 1;
  if ((st = make_rows(s, rows, L.rows))) return st;
  return aa_scale(L, ls);
}

// What the launch writes on the device: `spx` pixels per output buffer in d_out; for a direct launch (z: the caller's
// buffers as the device sees them, else null) also the groups' completion counters.
int prepare_outputs(ctr_scene *s, RenderLaunch &L, size_t spx, const HostFrame *z) {
  if (!s->h_counters) HIP_TRY(hipHostMalloc((void **)&s->h_counters, 16 * sizeof(unsigned long long), hipHostMallocDefault));
  if (int st = grow(spx, s->out_px, {{(void **)&s->d_out, 7 * sizeof(float), false}})) return st;
  L.depth = s->d_out;
  L.color = s->d_out + spx;
  L.normal = s->d_out + 4 * spx;
  if (!z) return CTR_OK;
  const size_t groups = (size_t)ctr_staging_groups(L);
  if (int st = grow(groups, s->groups_cap, {{(void **)&s->d_groups, sizeof(uint32_t), false}, {(void **)&s->h_groups, sizeof(uint32_t), true}})) return st;
  // cleared at the head of EVERY direct launch (a few microseconds): whatever an earlier launch left behind — one
  // that faulted or was cut short included — this one starts from zero
  HIP_TRY(hipMemsetAsync(s->d_groups, 0, groups * sizeof(uint32_t), nullptr));
  L.host_depth = z->depth;
  L.host_color = z->color3;
  L.host_normal = z->normal3;
  L.group_done = s->d_groups;
  return CTR_OK;
}

// Copy-out (the reference does 3·h row-wise copies, kernel.hpp:110-114).  Page-locked destinations
// (ctr_frame_alloc, hipHostMalloc, hipHostRegister) are written by direct DMA queued behind the kernel:
// ONE transfer when the three buffers are the consecutive parts of one block, else one per buffer.
// Pageable destinations go through the runtime's staged copy, one call per buffer.
int copy_out(ctr_scene *s, const RenderLaunch &L, const HostFrame &o, size_t px) {
  const bool packed = o.depth && o.color3 == o.depth + px && o.normal3 == o.color3 + 3 * px;
  if (packed && is_pinned(o.depth) && is_pinned(o.normal3 + 3 * px - 1)) {
    HIP_TRY(hipMemcpyAsync(o.depth, s->d_out, sizeof(float) * 7 * px, hipMemcpyDeviceToHost, nullptr));
  } else {
    auto out = [&](float *dst, const float *src, size_t n) -> hipError_t {
      if (!dst) return hipSuccess;
      if (is_pinned(dst) && is_pinned(dst + n - 1)) return hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToHost, nullptr);
      return hipMemcpy(dst, src, sizeof(float) * n, hipMemcpyDeviceToHost);
    };
    HIP_TRY(out(o.depth, L.depth, px));
    HIP_TRY(out(o.color3, L.color, 3 * px));
    HIP_TRY(out(o.normal3, L.normal, 3 * px));
  }
  if (o.uv2) HIP_TRY(hipMemcpy(o.uv2, s->d_uv, sizeof(float) * 2 * px, hipMemcpyDeviceToHost));
  return CTR_OK;
}

// ---- display frames (include/cutrace_images.h) ----
// the caller's byte planes of ctr_render_images (null: not asked for)
struct HostImages { uint8_t *depth8, *color8, *normal8; };

// In place of copy_out: the frame the launch left in d_out is quantised behind it on the same stream, with the largest depth
// the launch itself accumulated in d_counters, and only the byte planes asked for leave the device: one copy per plane,
// queued where the destination is page-locked, staged by the runtime where it is not.
int images_out(ctr_scene *s, const RenderLaunch &L, const HostImages &o, size_t px) {
  if (int st = grow(px, s->img_px, {{(void **)&s->d_img, 9, false}})) return st;
  ImagesLaunch Q{};
  Q.n = px;
  Q.counters = s->d_counters;
  if (o.depth8) { Q.depth = L.depth; Q.depth8 = s->d_img; }
  if (o.color8) { Q.color = L.color; Q.color8 = s->d_img + 3 * px; }
  if (o.normal8) { Q.normal = L.normal; Q.normal8 = s->d_img + 6 * px; }
  if (int e = ctr_launch_images(Q, nullptr)) return hip_fail((hipError_t)e, "quantise kernel launch");
  auto out = [&](uint8_t *dst, const uint8_t *src) -> hipError_t {
    if (!dst) return hipSuccess;
    if (is_pinned(dst) && is_pinned(dst + 3 * px - 1)) return hipMemcpyAsync(dst, src, 3 * px, hipMemcpyDeviceToHost, nullptr);
    return hipMemcpy(dst, src, 3 * px, hipMemcpyDeviceToHost);
  };
  HIP_TRY(out(o.depth8, Q.depth8));
  HIP_TRY(out(o.color8, Q.color8));
  HIP_TRY(out(o.normal8, Q.normal8));
  return CTR_OK;
}

// A direct launch is over and h_groups holds its counters: did the whole frame reach the caller's buffers?
int check_delivery(ctr_scene *s, const RenderLaunch &L, const HostFrame &o, size_t spx, size_t n_groups) {
  // every group of tiles must have counted all its tiles, or its pixels never left for the caller's buffers
  // (how many tiles a group has is the kernel's business — its tile shape is a build option: ctr_group_tile_count)
  size_t missing = 0;
  for (size_t g = 0; g < n_groups; g++)
    if (s->h_groups[g] != ctr_group_tile_count(L, g)) missing++;
  if (missing) {
    s->order_valid = false;  // whatever order that launch ran in is not to be trusted
    return fail(CTR_E_DELIVERY, std::to_string(missing) + " of " + std::to_string(n_groups) +
                " tile groups were not delivered to the caller's buffers (incomplete launch); render again");
  }
  if (!getenv("CUTRACE_VERIFY_DELIVERY")) return CTR_OK;
  // Debug aid for the kernel's own delivery (render_kernel.hip "Host delivery" relies on write-through stores and
  // scoped loads instead of fences): the tile-major staging copy of the frame is still on the device — fetch it
  // and compare every pixel with what arrived in the caller's buffers.
  std::vector<float> stg(7 * spx);
  HIP_TRY(hipMemcpy(stg.data(), s->d_out, sizeof(float) * 7 * spx, hipMemcpyDeviceToHost));
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
// returned in `stats` and `aabb_tris`.
int report(ctr_scene *s, const RenderLaunch &L, std::chrono::high_resolution_clock::time_point t0, ctr_render_stats *stats,
           unsigned long long *aabb_tris) {
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  unsigned long long cnt[16];
  memcpy(cnt, s->h_counters, sizeof(cnt));
  memcpy(s->last_cnt, cnt, sizeof(cnt));
  if (s->user_variant & CTR_VAR_STATS)
    fprintf(stderr, "cutrace_amd stats: wave_casts=%llu nodes=%llu tri_prefilter=%llu tri_exact=%llu mesh_entries=%llu "
                    "active_lanes=%llu node_lanes=%llu prefilter_lanes=%llu exact_lanes=%llu lane_max_nodes=%llu "
                    "lane_max_tris=%llu kernel_ms=%.3f\n", cnt[4], cnt[5],
            cnt[6], cnt[7], cnt[8], cnt[9], cnt[10], cnt[11], cnt[12], cnt[13], cnt[14], ms);
  if (aabb_tris) *aabb_tris = cnt[2];
  if (cnt[13] && !(s->user_variant & CTR_VAR_STATS))  // CTR_TIMING diagnostic build: share of the waves' lifetime
    fprintf(stderr, "cutrace_amd timing (%% of wave cycles): cast_setup=%.1f planes=%.1f object_loop=%.1f tlas+aabb=%.1f "
                    "mesh_setup=%.1f bvh_nodes=%.1f leaves=%.1f cont_mode=%.1f cont_rest=%.1f | wave_total=%llu kernel_ms=%.3f\n",
            100.0 * cnt[4] / cnt[13], 100.0 * cnt[5] / cnt[13], 100.0 * cnt[6] / cnt[13], 100.0 * cnt[7] / cnt[13],
            100.0 * cnt[8] / cnt[13], 100.0 * cnt[9] / cnt[13], 100.0 * cnt[10] / cnt[13], 100.0 * cnt[11] / cnt[13],
            100.0 * cnt[12] / cnt[13], cnt[13], ms);
  auto t1 = std::chrono::high_resolution_clock::now();
  if (stats) {
    stats->kernel_ms = ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    stats->ray_count = cnt[0];
    stats->rows = L.rows.n_rows >> L.ss_log2;  // (output rows)
    stats->max_depth = depth_of_counter(cnt[1]);
    stats->reserved = 0;
  }
  return CTR_OK;
}

}  // namespace

extern "C" {

int ctr_abi_version(void) { return CTR_ABI_VERSION; }
const char *ctr_last_error(void) { return g_err.c_str(); }

int ctr_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return -hip_fail(e, "hipGetDeviceCount");
  return n;
}

int ctr_scene_create(const ctr_scene_desc *d, int device, ctr_scene **out) {
  if (!d || !out) return fail(CTR_E_INVALID, "ctr_scene_create: null argument");
  *out = nullptr;
  std::string err;
  if (int st = validate_desc(*d, err)) return fail(st, err);

  create_stamp(nullptr);  // CUTRACE_DEBUG_CREATE=1: where the call spends its time (stderr)
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(CTR_E_NO_DEVICE, "no HIP device available (and there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CTR_E_INVALID, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  create_stamp("device check");

  FlatScene F;
  if (int st = flatten_scene(*d, F, err)) return fail(st, err);
  auto *s = new ctr_scene();
  s->device = device;
  s->cam = to_dcam(d->cam);
  if (const char *e = getenv("CUTRACE_NO_SCENE_HEAD")) s->no_scene_head = atoi(e) != 0;  // A/B and tests: every record by pointer

  hipError_t er = hipSuccess;
  for (const SceneArray &a : scene_arrays(s, F)) {
    // never hand the kernel a null base pointer: allocate at least one element's worth
    // (and 256 bytes beyond the end: the leaf loop requests the three cache lines after a leaf's first triangle ahead
    //  of their use, whether the leaf has that many triangles or not — render_kernel.hip, "touch")
    if (er == hipSuccess) er = hipMalloc(a.dev, (a.bytes ? a.bytes : 64) + 256);
    if (er == hipSuccess && a.bytes) er = hipMemcpy(*a.dev, a.host, a.bytes, hipMemcpyHostToDevice);
  }
  const size_t shard_bytes = (size_t)CTR_SHARDS * CTR_SHARD_WORDS * sizeof(unsigned long long);
  if (er != hipSuccess || (er = hipMalloc((void **)&s->d_cams, sizeof(DCam))) != hipSuccess ||
      (er = hipMemcpy(s->d_cams, &s->cam, sizeof(DCam), hipMemcpyHostToDevice)) != hipSuccess ||
      (er = hipMalloc((void **)&s->d_counters, 16 * sizeof(unsigned long long))) != hipSuccess ||
      (er = hipMalloc((void **)&s->d_shards, shard_bytes)) != hipSuccess || (er = hipMemset(s->d_shards, 0, shard_bytes)) != hipSuccess ||
      (er = hipEventCreate(&s->ev0)) != hipSuccess || (er = hipEventCreate(&s->ev1)) != hipSuccess) {
    ctr_scene_destroy(s);
    return hip_fail(er, "scene upload");
  }
  create_stamp("device allocation + upload");
  s->n_cams = 1;
  s->flat = std::move(F);
  s->h_cams.assign(1, s->cam);
  create_stamp("host copies");
  if (int st = refresh_linear_meshes(s)) {
    ctr_scene_destroy(s);
    return st;
  }
  create_stamp("guard records");
  *out = s;
  return CTR_OK;
}

int ctr_scene_set_cameras(ctr_scene *s, const ctr_camera *cams, uint32_t n) {
  if (!s || !cams || n == 0) return fail(CTR_E_INVALID, "ctr_scene_set_cameras: bad argument");
  std::vector<DCam> dc(n);
  for (uint32_t i = 0; i < n; i++) {
    if (cams[i].w != cams[0].w || cams[i].h != cams[0].h)
      return fail(CTR_E_INVALID, "ctr_scene_set_cameras: all cameras of a batch must share width and height");
    dc[i] = to_dcam(cams[i]);
  }
  if (dc[0].w == 0 || dc[0].h == 0) return fail(CTR_E_INVALID, "camera has zero width or height");
  std::lock_guard<std::mutex> lk(s->mtx);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());  // no launch may still be reading the old array
  DCam *nd = nullptr;
  HIP_TRY(hipMalloc((void **)&nd, sizeof(DCam) * n));
  hipError_t e = hipMemcpy(nd, dc.data(), sizeof(DCam) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(nd); return hip_fail(e, "camera upload"); }
  if (s->d_cams) (void)hipFree(s->d_cams);
  s->d_cams = nd;
  s->n_cams = n;
  s->cams_epoch++;
  s->cam = dc[0];
  s->h_cams = dc;
  return refresh_linear_meshes(s);
}

void ctr_scene_destroy(ctr_scene *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (const SceneArray &a : scene_arrays(s, s->flat))
    if (*a.dev) (void)hipFree(*a.dev);
  for (void *p : {(void *)s->d_cams, (void *)s->d_out, (void *)s->d_uv, (void *)s->d_img, (void *)s->d_groups, (void *)s->d_counters, (void *)s->d_shards,
                  (void *)s->d_cost, (void *)s->d_order})
    if (p) (void)hipFree(p);
  if (s->h_counters) (void)hipHostFree(s->h_counters);
  if (s->h_groups) (void)hipHostFree(s->h_groups);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
}

int ctr_scene_size(const ctr_scene *s, uint64_t *w, uint64_t *h) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  if (w) *w = s->cam.w;
  if (h) *h = s->cam.h;
  return CTR_OK;
}

int ctr_scene_set_size(ctr_scene *s, uint64_t w, uint64_t h) {
  if (!s || w == 0 || h == 0 || w > 0x7FFFFFFFull || h > 0x7FFFFFFFull) return fail(CTR_E_INVALID, "bad size");
  std::lock_guard<std::mutex> lk(s->mtx);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<DCam> dc(s->n_cams);
  HIP_TRY(hipMemcpy(dc.data(), s->d_cams, sizeof(DCam) * s->n_cams, hipMemcpyDeviceToHost));
  for (DCam &c : dc) { c.w = (uint32_t)w; c.h = (uint32_t)h; }
  HIP_TRY(hipMemcpy(s->d_cams, dc.data(), sizeof(DCam) * s->n_cams, hipMemcpyHostToDevice));
  s->cam.w = (uint32_t)w;
  s->cam.h = (uint32_t)h;
  s->cams_epoch++;
  return CTR_OK;
}

int ctr_set_variant(ctr_scene *s, uint32_t bits) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  constexpr uint32_t KNOWN = CTR_VAR_NO_PREFILTER | CTR_VAR_NO_ANYHIT | CTR_VAR_NO_CLUSTER | CTR_VAR_STATS | CTR_VAR_EXACT_POW |
                             CTR_VAR_NO_REORDER | CTR_VAR_NO_OCC6 | CTR_VAR_NO_DIRECT | CTR_VAR_IMAGE_ORDER_FIRST | CTR_VAR_MERGE | CTR_VAR_IGNORE_TRANSPARENT;
  if (bits & ~KNOWN) return fail(CTR_E_INVALID, "ctr_set_variant: unknown variant bits " + std::to_string(bits & ~KNOWN));
  s->user_variant = bits;
  if ((bits & CTR_VAR_MERGE) && s->flat.merged.reserved && !s->flat.merged.built) {
    std::lock_guard<std::mutex> lk(s->mtx);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    return build_merged_tree(s);
  }
  return CTR_OK;
}

// ss_log2 != 0: one supersampled frame (ctr_render_device_aa, whose checks have passed)
// lens: the primary rays are the caller's (ctr_render_device_lens, whose checks have passed), with ss_log2 one per sample
static int render_device(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, uint32_t first_frame,
                         uint32_t n_frames, uint64_t frame_stride_px, uint32_t part_stride, void *d_depth,
                         void *d_color3, void *d_normal3, void *d_counters, void *hip_stream, uint32_t ss_log2,
                         const ctr_lens *lens = nullptr) {
  int st = check_args(s, bounces);
  if (st) return st;
  if (!d_depth || !d_color3 || !d_normal3) return fail(CTR_E_INVALID, "null output buffer");
  const KernelEntry entry = lens ? (ss_log2 ? KE_DEVICE_LENS_SS : KE_DEVICE_LENS) : (ss_log2 ? KE_DEVICE_SS : KE_DEVICE);
  const KernelChoice choice = choose_kernel(kernel_facts(s, entry, bounces, false));
  if (choice.reject == KR_IGNTR_DEVICE) return fail(CTR_E_INVALID, "CTR_VAR_IGNORE_TRANSPARENT: host-buffer calls only (ctr_render, ctr_render_uv)");
  if (n_frames == 0 || first_frame >= s->n_cams || n_frames > s->n_cams - first_frame)
    return fail(CTR_E_INVALID, "frame range exceeds the cameras set with ctr_scene_set_cameras");
  if ((st = use_device(s))) return st;
  RenderLaunch L{};
  fill_launch(s, L);
  if ((st = make_rows(s, rows, L.rows))) return st;
  if (part_stride && L.rows.n_parts > 1) {
    // parts rotate: size the per-frame tile grid for the largest part
    L.rows.part_stride = part_stride % L.rows.n_parts;
    uint32_t cap = 0;
    for (uint32_t p = 0; p < L.rows.n_parts; p++) {
      ctr_rows rp = *rows;
      rp.part = p;
      DRows tmp{};
      if ((st = make_rows(s, &rp, tmp))) return st;
      cap = tmp.n_rows > cap ? tmp.n_rows : cap;
    }
    L.rows.n_rows = cap;
  }
  if (n_frames > 1 && frame_stride_px < (uint64_t)L.rows.n_rows * s->cam.w)
    return fail(CTR_E_INVALID, "frame_stride_px smaller than one frame's rows");
  L.first_frame = first_frame;
  L.n_frames = n_frames;
  L.frame_stride_px = frame_stride_px;
  L.fudge = fudge;
  L.bounces = bounces;
  L.depth = (float *)d_depth;
  L.color = (float *)d_color3;
  L.normal = (float *)d_normal3;
  L.counters = (unsigned long long *)d_counters;
  L.variant = choice.kv;
  if (lens) {
    L.ray_origin = lens->d_origin;
    L.ray_dir = lens->d_dir;
    L.ray_ambient = lens->ambient;
  }
  if (ss_log2 && (st = aa_scale(L, ss_log2))) return st;
  set_root_and_head(s, L, choice.merged);
  {
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((st = attach_order(s, L, false))) return st;
    s->last_kernel = L.variant;
  }
  int e = ctr_launch_render(L, hip_stream);
  if (e) return hip_fail((hipError_t)e, "render kernel launch");
  return CTR_OK;
}

int ctr_render_device_batch(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, uint32_t first_frame,
                            uint32_t n_frames, uint64_t frame_stride_px, uint32_t part_stride, void *d_depth,
                            void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  return render_device(s, fudge, bounces, rows, first_frame, n_frames, frame_stride_px, part_stride, d_depth, d_color3, d_normal3,
                       d_counters, hip_stream, 0);
}

int ctr_render_device_aa(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, void *d_depth,
                         void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  uint32_t ls = 0;
  if (int st = aa_precheck(s, KE_DEVICE_SS, bounces, samples, rows, ls)) return st;
  return render_device(s, fudge, bounces, rows, 0, 1, 0, 0, d_depth, d_color3, d_normal3, d_counters, hip_stream, ls);
}

// include/cutrace_lens.h.  Every check comes before the GPU is touched (hipPointerGetAttributes asks the runtime, no device work)
int ctr_render_device_lens(ctr_scene *s, float fudge, int bounces, const ctr_lens *lens, const ctr_rows *rows, void *d_depth,
                           void *d_color3, void *d_normal3, void *d_counters, void *hip_stream) {
  const std::string who = "ctr_render_device_lens: ";
  int st = check_args(s, bounces);
  if (st) return st;
  if (!lens) return fail(CTR_E_INVALID, who + "null lens");
  if (!lens->d_origin || !lens->d_dir) return fail(CTR_E_INVALID, who + "null rays");
  if (!d_depth || !d_color3 || !d_normal3) return fail(CTR_E_INVALID, who + "null output buffer");
  const uint32_t samples = lens->samples;
  if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
    return fail(CTR_E_INVALID, who + "samples must be 1, 2, 4 or 8 per axis, got " + std::to_string(samples));
  if (choose_kernel(kernel_facts(s, samples > 1 ? KE_DEVICE_LENS_SS : KE_DEVICE_LENS, bounces, false)).reject == KR_LENS)
    return fail(CTR_E_INVALID, who + "no build for CTR_VAR_STATS, CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER or CTR_VAR_NO_CLUSTER");
  uint32_t ls = 0;
  if ((st = aa_precheck(s, KE_DEVICE_SS, bounces, samples, rows, ls))) return st;  // (the size limits of the sample frame)
  // (w, h <= 2^32 / s each, s*s <= 64: the product fits 64 bits)
  const uint64_t want = ((uint64_t)s->cam.w << ls) * ((uint64_t)s->cam.h << ls);
  if (lens->n_rays != want)
    return fail(CTR_E_INVALID, who + "n_rays is " + std::to_string(lens->n_rays) + ", the " + std::to_string(samples) + " x " + std::to_string(samples) +
                                   " samples of the " + std::to_string(s->cam.w) + " x " + std::to_string(s->cam.h) + " frame are " + std::to_string(want));
  const void *const ptrs[] = {lens->d_origin, lens->d_dir};
  const char *const names[] = {"d_origin", "d_dir"};
  if ((st = check_device_pointers(s->device, who, ptrs, names, 2))) return st;
  return render_device(s, fudge, bounces, rows, 0, 1, 0, 0, d_depth, d_color3, d_normal3, d_counters, hip_stream, ls, lens);
}

int ctr_render_device(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, void *d_depth, void *d_color3,
                      void *d_normal3, void *d_counters, void *hip_stream) {
  return ctr_render_device_batch(s, fudge, bounces, rows, 0, 1, 0, 0, d_depth, d_color3, d_normal3, d_counters, hip_stream);
}

// ss_log2 != 0: a supersampled frame (ctr_render_aa, whose checks have passed): rows, px and the buffers are the output's
// images: the frame leaves as byte planes (ctr_render_images): chosen for as a render into pageable memory, `out` empty
static int render_host(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, const HostFrame &out, ctr_render_stats *stats,
                       bool count, unsigned long long *aabb_tris, uint32_t ss_log2 = 0, const HostImages *images = nullptr) {
  auto t0 = std::chrono::high_resolution_clock::now();
  int st = check_args(s, bounces);
  if (st) return st;
  std::lock_guard<std::mutex> lk(s->mtx);
  HIP_TRY(hipSetDevice(s->device));
  RenderLaunch L{};
  fill_launch(s, L);
  if ((st = make_rows(s, rows, L.rows))) return st;
  const size_t px = (size_t)L.rows.n_rows * s->cam.w;
  HostFrame z{};
  if (ss_log2 && (st = aa_scale(L, ss_log2))) return st;
  // an empty selection launches nothing and has no fourth output: it is chosen for as a plain render
  KernelFacts facts = kernel_facts(s, count ? KE_COUNT : ss_log2 ? KE_HOST_SS : out.uv2 && px ? KE_UV : KE_HOST, bounces, !images);
  if (!px) facts.user &= ~CTR_VAR_IGNORE_TRANSPARENT;
  KernelChoice choice = choose_kernel(facts);
  // (the caller's buffers are looked at only where everything else allows delivery by the kernel)
  if (choice.direct && !device_visible(out, px, z)) {
    facts.deliverable = false;
    choice = choose_kernel(facts);
  }
  const bool direct = choice.direct;
  const size_t spx = direct ? (size_t)ctr_staging_pixels(L) : (px ? px : 1);  // pixels per output buffer on the device
  L.fudge = fudge;
  L.bounces = bounces;
  if ((st = prepare_outputs(s, L, spx, direct ? &z : nullptr))) return st;
  L.counters = s->d_counters;
  if (choice.reject == KR_UV_STATS) return fail(CTR_E_INVALID, "ctr_render_uv / CTR_VAR_IGNORE_TRANSPARENT: not with the counting / statistics variants");
  L.variant = s->last_kernel = choice.kv;
  if (L.variant & KV_UV) {
    if ((st = grow(px, s->uv_px, {{(void **)&s->d_uv, 2 * sizeof(float), false}}))) return st;
    L.uv = s->d_uv;
  }
  set_root_and_head(s, L, choice.merged);
  if ((st = attach_order(s, L, count))) return st;
  HIP_TRY(hipMemsetAsync(s->d_counters, 0, 16 * sizeof(unsigned long long), nullptr));
  HIP_TRY(hipEventRecord(s->ev0, nullptr));
  int e = ctr_launch_render(L, nullptr);
  if (e) return hip_fail((hipError_t)e, "render kernel launch");
  HIP_TRY(hipEventRecord(s->ev1, nullptr));
  if (px && !direct && (st = images ? images_out(s, L, *images, px) : copy_out(s, L, out, px))) return st;
  HIP_TRY(hipMemcpyAsync(s->h_counters, s->d_counters, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr));
  const size_t n_groups = direct ? (size_t)ctr_staging_groups(L) : 0;
  if (direct) HIP_TRY(hipMemcpyAsync(s->h_groups, s->d_groups, n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (direct && (st = check_delivery(s, L, out, spx, n_groups))) return st;
  return report(s, L, t0, stats, aabb_tris);
}

int ctr_render(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, float *depth, float *color3,
               float *normal3, ctr_render_stats *stats) {
  return render_host(s, fudge, bounces, rows, {depth, color3, normal3, nullptr}, stats, false, nullptr);
}

int ctr_render_aa(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, float *depth, float *color3,
                  float *normal3, ctr_render_stats *stats) {
  uint32_t ls = 0;
  if (int st = aa_precheck(s, KE_HOST_SS, bounces, samples, rows, ls)) return st;
  return render_host(s, fudge, bounces, rows, {depth, color3, normal3, nullptr}, stats, false, nullptr, ls);
}

// include/cutrace_images.h
int ctr_render_images(ctr_scene *s, float fudge, int bounces, uint32_t samples, const ctr_rows *rows, uint8_t *depth8,
                      uint8_t *color8, uint8_t *normal8, ctr_render_stats *stats) {
  if (!depth8 && !color8 && !normal8) return fail(CTR_E_INVALID, "ctr_render_images: no destination plane");
  uint32_t ls = 0;
  if (int st = aa_precheck(s, KE_HOST_SS, bounces, samples, rows, ls)) return st;
  const HostImages images{depth8, color8, normal8};
  return render_host(s, fudge, bounces, rows, {}, stats, false, nullptr, ls, &images);
}

int ctr_quantise_device(int device, const ctr_image_planes *p, void *hip_stream) {
  const std::string who = "ctr_quantise_device: ";
  if (!p) return fail(CTR_E_INVALID, who + "null planes");
  if (p->reserved) return fail(CTR_E_INVALID, who + "reserved must be 0");
  const void *const ptrs[] = {p->d_depth, p->d_color3, p->d_normal3, p->d_depth8, p->d_color8, p->d_normal8, p->d_counters};
  const char *const names[] = {"d_depth", "d_color3", "d_normal3", "d_depth8", "d_color8", "d_normal8", "d_counters"};
  for (int k = 0; k < 3; k++)
    if (!ptrs[k] != !ptrs[3 + k])
      return fail(CTR_E_INVALID, who + (ptrs[k] ? names[k] : names[3 + k]) + " without " + (ptrs[k] ? names[3 + k] : names[k]));
  if (!p->d_depth && !p->d_color3 && !p->d_normal3) return fail(CTR_E_INVALID, who + "no plane");
  if (p->n_pixels == 0) return CTR_OK;
  if (int st = check_device_pointers(device, who, ptrs, names, 7, ("device " + std::to_string(device)).c_str())) return st;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != device) HIP_TRY(hipSetDevice(device));
  const ImagesLaunch Q{p->n_pixels, p->d_depth, p->d_color3, p->d_normal3, p->d_depth8, p->d_color8, p->d_normal8,
                       (const unsigned long long *)p->d_counters, p->max_depth};
  if (int e = ctr_launch_images(Q, hip_stream)) return hip_fail((hipError_t)e, "quantise kernel launch");
  return CTR_OK;
}

int ctr_render_uv(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, float *depth, float *color3,
                  float *normal3, float *uv2, ctr_render_stats *stats) {
  if (!uv2) return fail(CTR_E_INVALID, "ctr_render_uv: null uv buffer");
  return render_host(s, fudge, bounces, rows, {depth, color3, normal3, uv2}, stats, false, nullptr);
}

int ctr_debug_poison_next_order(ctr_scene *s) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  std::lock_guard<std::mutex> lk(s->mtx);
  s->poison_next_order = true;
  return CTR_OK;
}

int ctr_debug_last_kernel(ctr_scene *s, uint32_t *kv) {
  if (!s || !kv) return fail(CTR_E_INVALID, "ctr_debug_last_kernel: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *kv = s->last_kernel;
  return CTR_OK;
}

int ctr_last_counters(ctr_scene *s, uint64_t *out16) {
  if (!s || !out16) return fail(CTR_E_INVALID, "ctr_last_counters: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  for (int q = 0; q < 16; q++) out16[q] = s->last_cnt[q];
  return CTR_OK;
}

int ctr_tile_costs(ctr_scene *s, uint32_t *out, uint64_t capacity, uint64_t *n_tiles) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  std::lock_guard<std::mutex> lk(s->mtx);
  const uint64_t n = s->order_valid ? s->order_key[0] : 0;
  if (n_tiles) *n_tiles = n;
  if (out && n) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, s->d_cost, sizeof(uint32_t) * (n < capacity ? n : capacity), hipMemcpyDeviceToHost));
  }
  return CTR_OK;
}

int ctr_frame_alloc(uint64_t n_pixels, float **depth, float **color3, float **normal3) {
  if (!depth || !color3 || !normal3 || n_pixels == 0) return fail(CTR_E_INVALID, "ctr_frame_alloc: bad argument");
  float *p = nullptr;
  // portable + mapped: page-locked for, and visible to, every device of the process (whichever one is current now)
  HIP_TRY(hipHostMalloc((void **)&p, sizeof(float) * 7 * n_pixels, hipHostMallocPortable | hipHostMallocMapped));
  *depth = p;
  *color3 = p + n_pixels;
  *normal3 = p + 4 * n_pixels;
  return CTR_OK;
}

void ctr_frame_free(float *depth) {
  if (depth) (void)hipHostFree(depth);
}

int ctr_algorithmic_bytes(ctr_scene *s, float fudge, int bounces, const ctr_rows *rows, uint64_t *bytes,
                          uint64_t *ray_count) {
  ctr_render_stats stt{};
  unsigned long long aabb = 0;
  int st = render_host(s, fudge, bounces, rows, {}, &stt, true, &aabb);
  if (st) return st;
  // 56·N_obj per ray_cast + 48·N_tri per AABB-hit mesh + 28 B per pixel written
  if (bytes) *bytes = 56ull * s->flat.objs.size() * stt.ray_count + 48ull * aabb + 28ull * stt.rows * s->cam.w;
  if (ray_count) *ray_count = stt.ray_count;
  return CTR_OK;
}

}  // extern "C"
