// ctr_scene.cpp — the scene handle of include/cutrace_amd.h on the gfx950 device: its lifetime, the uploads, the guard refresh and
// the merged tree, cameras and size, page-locked frames, and what ctr_internal.h declares for every host translation unit.
// The render path on top of the handle is ctr_render.cpp.
//
// Replaces the host half of the reference's hot path:
//   cpu_to_gpu::convert          inc/cpu_to_gpu.hpp:188-198  → ctr_scene_create (flatten_scene, scene_flatten.cpp, then one
//                                                               flat upload, hipMalloc + hipMemcpy, no managed memory)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ctr_internal.h"
#include "cutrace_amd.h"
#include "guard.h"
#include "scene_device.h"
#include "scene_flatten.h"

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

MemKind memory_kind(const void *p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // plain malloc'ed memory: "invalid value", not an error of ours or of the stream
    return {MemKind::HOST_OTHER, 0};
  }
  if (at.type == hipMemoryTypeDevice) return {MemKind::DEVICE, at.device};
  if (at.type == hipMemoryTypeHost) return {MemKind::HOST_PINNED, 0};
  return {at.type == hipMemoryTypeUnregistered ? MemKind::HOST_OTHER : MemKind::ELSEWHERE, 0};
}

int check_device_pointers(int device, const std::string &who, const NamedPtr *ptrs, size_t n, const char *whose) {
  for (size_t k = 0; k < n; k++) {
    if (!ptrs[k].p) continue;
    const MemKind m = memory_kind(ptrs[k].p);
    if (m.kind != MemKind::DEVICE || m.device != device)
      return fail(CTR_E_INVALID, who + ptrs[k].name + " is not device memory of " + whose);
  }
  return CTR_OK;
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
// Any other destination: device buffers + copies (ctr_render.cpp copy_out).
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

int GrowBuf::grow(size_t n, size_t keep) {
  if (n <= cap) return CTR_OK;
  if (keep > cap) keep = cap;  // (there is no more)
  const size_t bytes = n * elem + tail;
  void *q = nullptr;
  hipError_t e = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
  if (e != hipSuccess) return hip_fail(e, pinned ? "hipHostMalloc" : "hipMalloc");
  if (keep) e = hipMemcpy(q, p, keep * elem, pinned ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice);
  if (e != hipSuccess) {
    (void)(pinned ? hipHostFree(q) : hipFree(q));
    return hip_fail(e, "copy into the larger array");
  }
  release();
  p = q;
  cap = n;
  return CTR_OK;
}
void GrowBuf::release() {
  if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
  p = nullptr;
  cap = 0;
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

// The scene's ten device arrays, each ONCE: the member of the handle that owns it (its record size is the unit of a DirtyRange),
// its host copy (scene_flatten.h FlatScene) and the bytes of that, and the key under which a DirtyRange names it (-1: never
// edited through one after the upload).  ctr_scene_create uploads and upload_dirty re-uploads by this table.  F: s->flat, or
// what ctr_scene_create is about to move there.
struct SceneArray { GrowBuf *dev; const void *host; size_t bytes; int dirty; };
std::vector<SceneArray> scene_arrays(ctr_scene *s, const FlatScene &F) {
  auto row = [](GrowBuf &dev, const auto &v, int dirty = -1) { return SceneArray{&dev, v.data(), v.size() * sizeof(v[0]), dirty}; };
  return {row(s->d_objs, F.objs, DirtyRange::OBJS), row(s->d_oloop, F.oloop, DirtyRange::OLOOP), row(s->d_meshes, F.meshes, DirtyRange::MESHES),
          row(s->d_planes, F.planes, DirtyRange::PLANES), row(s->d_tris, F.tris, DirtyRange::TRIS), row(s->d_nodes, F.nodes, DirtyRange::NODES),
          row(s->d_nodes4, F.nodes4, DirtyRange::NODES4), row(s->d_gnorm, F.gn, DirtyRange::GNORM),
          row(s->d_lights, F.lights), row(s->d_mats, F.mats)};
}

}  // namespace

// the device receives the records a host-side edit changed (scene_flatten.h DirtyRange), in the order of the list
int upload_dirty(ctr_scene *s, const std::vector<DirtyRange> &dirty) {
  const std::vector<SceneArray> arrays = scene_arrays(s, s->flat);
  for (const DirtyRange &r : dirty)
    for (const SceneArray &a : arrays) {
      if (a.dirty != (int)r.array || !r.count) continue;
      const size_t rec = a.dev->elem;
      const void *src = r.payload.empty() ? (const char *)a.host + r.begin * rec : (const char *)r.payload.data();
      HIP_TRY(hipMemcpy(a.dev->as<char>() + r.begin * rec, src, r.count * rec, hipMemcpyHostToDevice));
    }
  return CTR_OK;
}

namespace {

// Plane-probe pairs from which the guard's scan runs on the device.  Below it the host loop is cheaper than a launch, two
// small copies and a wait.  Measured on one MI355X over mesh size at the bunny room's 30 probes (profiles/scene_edit/edit.txt
// (c)): the device path costs 0.034 .. 0.039 ms whatever the size, the host path 0.040 ms at 500 triangles and 0.057 ms at
// 1000, the first size at which the device's median wins by more than the two min .. max spreads together.
constexpr uint64_t CTR_GUARD_SCAN_MIN_WORK = 30000;

// CUTRACE_GUARD_SCAN=host|device overrides the threshold (read per call: one process can use both)
bool scan_on_device(uint64_t n_planes, size_t n_probes) {
  if (n_planes == 0 || n_planes > 0xFFFFFFFFull || n_probes == 0) return false;
  if (const char *e = getenv("CUTRACE_GUARD_SCAN")) {
    if (!strcmp(e, "host")) return false;
    if (!strcmp(e, "device")) return true;
  }
  return n_planes * n_probes >= CTR_GUARD_SCAN_MIN_WORK;
}

// The device half of a plan: the flat plane array (uploaded whole at the first scan; ctr_scene_update_mesh keeps it current), the
// probes uploaded, one launch, the words back through the page-locked buffer in one wait.  *words: where they are.
int device_scan(ctr_scene *s, const GuardProbes &P, uint64_t n_planes, const uint64_t **words) {
  const FlatScene &F = s->flat;
  const uint64_t n_words = guard_scan_words(n_planes);
  if (n_planes > s->scan_planes.cap) s->scan_planes_live = false;
  if (int st = s->scan_planes.reserve(n_planes)) return st;
  if (int st = s->scan_probes.reserve(P.probes.size())) return st;
  if (int st = reserve_both(s->scan_words, s->scan_back, n_words)) return st;
  uint64_t first = 0;
  for (const MeshGuard &g : F.guards) {
    if (!s->scan_planes_live && !g.planes.empty())
      HIP_TRY(hipMemcpyAsync(s->scan_planes.as<double>() + CTR_PLANE_DOUBLES * first, g.planes.data(), g.planes.size() * sizeof(double), hipMemcpyHostToDevice, nullptr));
    first += g.planes.size() / CTR_PLANE_DOUBLES;
  }
  s->scan_planes_live = true;
  HIP_TRY(hipMemcpyAsync(s->scan_probes.p, P.probes.data(), P.probes.size() * sizeof(GuardProbe), hipMemcpyHostToDevice, nullptr));
  if (int st = launched(ctr_launch_guard_scan(s->scan_planes.as<double>(), (uint32_t)n_planes, s->scan_probes.as<GuardProbe>(),
                                              (uint32_t)P.n_points, (uint32_t)P.probes.size(), s->scan_words.as<uint64_t>(), nullptr), "guard_scan launch"))
    return st;
  HIP_TRY(hipMemcpyAsync(s->scan_back.p, s->scan_words.p, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *words = s->scan_back.as<uint64_t>();
  return CTR_OK;
}

}  // namespace

int guard_planes_changed(ctr_scene *s, size_t gi, const double *src_dev) {
  if (!s->scan_planes_live) return CTR_OK;
  uint64_t first = 0;
  for (size_t i = 0; i < gi; i++) first += s->flat.guards[i].planes.size() / CTR_PLANE_DOUBLES;
  s->scan_planes_live = false;  // (until the copy is queued: a failure leaves the whole array to be uploaded again)
  HIP_TRY(hipMemcpyAsync(s->scan_planes.as<double>() + CTR_PLANE_DOUBLES * first, src_dev, s->flat.guards[gi].planes.size() * sizeof(double),
                         hipMemcpyDeviceToDevice, nullptr));
  s->scan_planes_live = true;
  return CTR_OK;
}

// The guard of the BVH culling (guard.cpp): at upload, whenever the cameras, the lights or the materials change and after a
// mesh update — plan, apply to the host copy, upload what changed.  Which side scans the planes is decided HERE alone.
int refresh_linear_meshes(ctr_scene *s, bool may_scan_on_device) {
  const GuardProbes P = guard_probes(s->flat, s->h_cams);
  const uint64_t n_planes = guard_plane_count(s->flat);
  const uint64_t *words = nullptr;  // null: plan_guards scans on the host
  if (may_scan_on_device && scan_on_device(n_planes, P.probes.size()))
    if (int st = device_scan(s, P, n_planes, &words)) return st;
  const GuardPlan plan = plan_guards(s->flat, P, words);
  const std::vector<DirtyRange> dirty = apply_guards(s->flat, plan);
  if (getenv("CUTRACE_DEBUG_GUARDS")) {
    size_t per_mesh = 0;
    for (const MeshGuard &g : s->flat.guards) per_mesh += g.guarded.size();
    fprintf(stderr, "cutrace_amd guards: %zu origins (eyes + mirror images), %zu mirrors, %zu guard records over %zu meshes, merged keys %zu, linear %d, scan on the %s\n",
            plan.n_origins, plan.n_mirrors, per_mesh, s->flat.guards.size(), plan.merged_keys.size(), (int)plan.any_linear, words ? "device" : "host");
  }
  return upload_dirty(s, dirty);
}

namespace {

// The merged tree of a scene that has room for it (scene_flatten.h Merged): built, uploaded, guarded.
int build_merged_tree(const Edit &edit) {
  ctr_scene *s = edit.s;
  const std::vector<DirtyRange> dirty = ::build_merged_tree(s->flat);
  if (dirty.empty()) return CTR_OK;
  if (int st = upload_dirty(s, dirty)) {
    s->flat.merged.built = false;  // (the device never got it: the next ctr_set_variant builds it again)
    return st;
  }
  return edit.end({}, false);  // (the tree went up above, where a failure has a consequence of its own)
}

// ctr_scene_create's device half: every array of F, the one camera, the counters and the zeroed shards, the two events
int upload_scene(ctr_scene *s, const FlatScene &F) {
  for (const SceneArray &a : scene_arrays(s, F)) {
    const size_t n = a.bytes / a.dev->elem;
    if (int st = a.dev->reserve(n ? n : 1)) return st;  // (never hand the kernel a null base pointer)
    if (a.bytes) HIP_TRY(hipMemcpy(a.dev->p, a.host, a.bytes, hipMemcpyHostToDevice));
  }
  const size_t shard_words = (size_t)CTR_SHARDS * CTR_SHARD_WORDS;
  if (int st = s->d_cams.reserve(1)) return st;
  HIP_TRY(hipMemcpy(s->d_cams.p, &s->cam, sizeof(DCam), hipMemcpyHostToDevice));
  if (int st = s->d_counters.reserve(16)) return st;
  if (int st = s->d_shards.reserve(shard_words)) return st;
  HIP_TRY(hipMemset(s->d_shards.p, 0, shard_words * sizeof(unsigned long long)));
  HIP_TRY(hipEventCreate(&s->ev0));
  HIP_TRY(hipEventCreate(&s->ev1));
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
  s->no_scene_head = env_switch("CUTRACE_NO_SCENE_HEAD");    // every record by pointer
  s->no_shape_build = env_switch("CUTRACE_NO_SHAPE_BUILD");  // the general build of every launch
  s->no_wall_skip = env_switch("CUTRACE_NO_WALL_SKIP");      // no shadow trip skips its plane tests
  s->no_dark_skip = env_switch("CUTRACE_NO_DARK_SKIP");      // no shadow cast is left out for a light that cannot change the pixel
  s->no_opaque_build = env_switch("CUTRACE_NO_OPAQUE_BUILD");  // the parent instantiation of every one-mesh launch
  s->no_phase_split = env_switch("CUTRACE_NO_PHASE_SPLIT");     // the opaque builds as they are without their phased twins

  if (int st = upload_scene(s, F)) {
    ctr_scene_destroy(s);
    return hip_fail((hipError_t)(st - CTR_E_HIP_BASE), "scene upload");  // (every step of it is a call of the runtime)
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
  const Edit edit(s);
  if (int st = edit.begin()) return st;
  // the new array is complete before the old one is released: a failure leaves the old cameras
  GrowBuf fresh(sizeof(DCam));
  if (int st = fresh.grow(n, 0)) return st;
  const hipError_t e = hipMemcpy(fresh.p, dc.data(), sizeof(DCam) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "camera upload");
  s->d_cams.swap(fresh);  // (`fresh` takes the old array with it)
  s->n_cams = n;
  s->cams_epoch++;
  s->cam = dc[0];
  s->h_cams = dc;
  return edit.end({}, false);
}

void ctr_scene_destroy(ctr_scene *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);  // (the memory is released by the handle's members: delete, below)
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;  // (every GrowBuf of the handle releases its memory here)
}

int ctr_scene_size(const ctr_scene *s, uint64_t *w, uint64_t *h) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  if (w) *w = s->cam.w;
  if (h) *h = s->cam.h;
  return CTR_OK;
}

int ctr_scene_set_size(ctr_scene *s, uint64_t w, uint64_t h) {
  if (!s || w == 0 || h == 0 || w > 0x7FFFFFFFull || h > 0x7FFFFFFFull) return fail(CTR_E_INVALID, "bad size");
  const Edit edit(s);
  if (int st = edit.begin()) return st;
  std::vector<DCam> dc(s->n_cams);
  HIP_TRY(hipMemcpy(dc.data(), s->d_cams.p, sizeof(DCam) * s->n_cams, hipMemcpyDeviceToHost));
  for (DCam &c : dc) { c.w = (uint32_t)w; c.h = (uint32_t)h; }
  HIP_TRY(hipMemcpy(s->d_cams.p, dc.data(), sizeof(DCam) * s->n_cams, hipMemcpyHostToDevice));
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
  const Edit edit(s);
  s->user_variant = bits;  // (kept also when the build below fails)
  if (!(bits & CTR_VAR_MERGE) || !s->flat.merged.reserved || s->flat.merged.built) return CTR_OK;
  if (int st = edit.begin()) return st;
  return build_merged_tree(edit);
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

int ctr_debug_last_kernel(ctr_scene *s, uint32_t *kv) {
  if (!s || !kv) return fail(CTR_E_INVALID, "ctr_debug_last_kernel: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *kv = s->last_kernel;
  return CTR_OK;
}

int ctr_debug_last_shape(ctr_scene *s, uint32_t *shape) {
  if (!s || !shape) return fail(CTR_E_INVALID, "ctr_debug_last_shape: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *shape = s->last_shape;
  return CTR_OK;
}

int ctr_debug_last_opaque(ctr_scene *s, uint32_t *opaque) {
  if (!s || !opaque) return fail(CTR_E_INVALID, "ctr_debug_last_opaque: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *opaque = s->last_opaque;
  return CTR_OK;
}

int ctr_debug_last_phased(ctr_scene *s, uint32_t *phased) {
  if (!s || !phased) return fail(CTR_E_INVALID, "ctr_debug_last_phased: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *phased = s->last_phased;
  return CTR_OK;
}

int ctr_debug_room_facts(ctr_scene *s, float *out5, uint32_t *lights) {
  if (!s || !out5 || !lights) return fail(CTR_E_INVALID, "ctr_debug_room_facts: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  for (int q = 0; q < 3; q++) out5[q] = s->last_room.c[q];
  out5[3] = s->last_room.r;
  out5[4] = s->last_room.delta;
  *lights = s->last_room.lights;
  return CTR_OK;
}

int ctr_debug_dark_skip(ctr_scene *s, uint32_t *word) {
  if (!s || !word) return fail(CTR_E_INVALID, "ctr_debug_dark_skip: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  *word = s->last_dark_skip;
  return CTR_OK;
}

int ctr_last_counters(ctr_scene *s, uint64_t *out16) {
  if (!s || !out16) return fail(CTR_E_INVALID, "ctr_last_counters: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  for (int q = 0; q < 16; q++) out16[q] = s->last_cnt[q];
  return CTR_OK;
}

}  // extern "C"
