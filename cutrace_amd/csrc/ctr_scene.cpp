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

int GrowBuf::reserve(size_t n) {
  if (n <= cap) return CTR_OK;
  release();
  HIP_TRY(pinned ? hipHostMalloc(&p, n * elem, hipHostMallocDefault) : hipMalloc(&p, n * elem));
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

// The scene's ten device arrays, each ONCE: its pointer in the handle's device scene (scene_device.h DScene), its host copy
// (scene_flatten.h FlatScene), the bytes of the whole array and of one record, and the key under which a DirtyRange names it
// (-1: never edited after the upload).  ctr_scene_create uploads, upload_dirty re-uploads and ctr_scene_destroy frees by this
// table.  F: s->flat, or what ctr_scene_create is about to move there.
struct SceneArray { void **dev; const void *host; size_t bytes, rec; int dirty; };
std::vector<SceneArray> scene_arrays(ctr_scene *s, const FlatScene &F) {
  auto row = [](auto &dev, const auto &v, int dirty = -1, size_t rec = 0) {
    return SceneArray{(void **)&dev, v.data(), v.size() * sizeof(v[0]), rec ? rec : sizeof(v[0]), dirty};
  };
  DScene &D = s->dev;
  return {row(D.objs, F.objs, DirtyRange::OBJS), row(D.oloop, F.oloop, DirtyRange::OLOOP), row(D.meshes, F.meshes, DirtyRange::MESHES),
          row(D.planes, F.planes, DirtyRange::PLANES), row(D.tris, F.tris, DirtyRange::TRIS), row(D.nodes, F.nodes, DirtyRange::NODES),
          row(D.nodes4, F.nodes4, DirtyRange::NODES4), row(D.gnorm, F.gn, DirtyRange::GNORM, 4 * sizeof(float)),
          row(D.lights, F.lights), row(D.mats, F.mats)};
}

}  // namespace

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
int build_merged_tree(ctr_scene *s) {
  const std::vector<DirtyRange> dirty = ::build_merged_tree(s->flat);
  if (dirty.empty()) return CTR_OK;
  if (int st = upload_dirty(s, dirty)) {
    s->flat.merged.built = false;  // (the device never got it: the next ctr_set_variant builds it again)
    return st;
  }
  return refresh_linear_meshes(s);
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
  if (const char *e = getenv("CUTRACE_NO_SHAPE_BUILD")) s->no_shape_build = atoi(e) != 0;  // A/B and tests: the general build of every launch
  s->no_wall_skip = wall_skip_switched_off();  // CUTRACE_NO_WALL_SKIP=1: A/B and tests: no shadow trip skips its plane tests

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
  for (void *p : {(void *)s->d_cams, (void *)s->d_counters, (void *)s->d_shards})
    if (p) (void)hipFree(p);
  if (s->h_counters) (void)hipHostFree(s->h_counters);
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

int ctr_debug_room_facts(ctr_scene *s, float *out5, uint32_t *lights) {
  if (!s || !out5 || !lights) return fail(CTR_E_INVALID, "ctr_debug_room_facts: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  for (int q = 0; q < 3; q++) out5[q] = s->last_room.c[q];
  out5[3] = s->last_room.r;
  out5[4] = s->last_room.delta;
  *lights = s->last_room.lights;
  return CTR_OK;
}

int ctr_last_counters(ctr_scene *s, uint64_t *out16) {
  if (!s || !out16) return fail(CTR_E_INVALID, "ctr_last_counters: null argument");
  std::lock_guard<std::mutex> lk(s->mtx);
  for (int q = 0; q < 16; q++) out16[q] = s->last_cnt[q];
  return CTR_OK;
}

}  // extern "C"
