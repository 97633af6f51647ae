// ctr_internal.h — what the host translation units of the library share: the scene handle and the error / device helpers.
//
// Defined in ctr_scene.cpp; used by ctr_scene.cpp (handle lifetime and uploads), ctr_render.cpp (the render path),
// tile_order_host.cpp (the tile scheduler's host half), ctr_rays.cpp (the ray queries) and ctr_multi.hip (the multi-device
// path).  Nothing here is part of the C-ABI.
#ifndef CUTRACE_AMD_CTR_INTERNAL_H
#define CUTRACE_AMD_CTR_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "cutrace_amd.h"
#include "guard_scan.h"
#include "lbvh.h"
#include "mesh_refit.h"
#include "scene_device.h"
#include "scene_flatten.h"
#include "tile_order_policy.h"

#pragma GCC visibility push(hidden)
// keeps `msg` for ctr_last_error(), prints it, returns `code`
int fail(int code, const std::string &msg);
// fail() with CTR_E_HIP_BASE + e and "<what>: <error name> (<error string>)"
int hip_fail(hipError_t e, const char *what);
#define HIP_TRY(expr)                                     \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) return hip_fail(_e, #expr);     \
  } while (0)
// the status of a launcher's return value (a hipError_t as int): CTR_OK, or hip_fail() with `what`
inline int launched(int e, const char *what) { return e ? hip_fail((hipError_t)e, what) : CTR_OK; }

// What kind of memory `p` names: the library's one hipPointerGetAttributes call.  A pointer the runtime does not know (plain
// malloc'ed memory: "invalid value", swallowed here, not an error of ours) is HOST_OTHER, as is memory it reports as
// unregistered; HOST_PINNED is hipHostMalloc / hipHostRegister memory; `device` is meaningful for DEVICE alone; ELSEWHERE is
// the rest (managed memory, arrays).
struct MemKind { enum Kind { HOST_PINNED, HOST_OTHER, DEVICE, ELSEWHERE } kind; int device; };
MemKind memory_kind(const void *p);
// is `p` page-locked host memory?  Then a D2H copy is one direct DMA.
inline bool is_pinned(const void *p) { return memory_kind(p).kind == MemKind::HOST_PINNED; }
// the device's address of page-locked host memory (false: not mapped for this device)
bool device_view(float *host, float **dev);
// the caller's buffers of a host-form render (uv2: ctr_render_uv only)
struct HostFrame { float *depth, *color3, *normal3, *uv2; };
// are the `px` pixels of all three buffers page-locked, first byte to last?
bool all_pinned(const HostFrame &o, size_t px);
// ... and mapped for the current device?  Then z = the same buffers as the device sees them, and its kernels can write them.
bool device_visible(const HostFrame &o, size_t px, HostFrame &z);
// counter word 1 of a launch as the float whose bits it carries: the largest finite depth, 0 if none (kernel.hpp:120-125)
inline float depth_of_counter(unsigned long long word) { const uint32_t bits = (uint32_t)word; float d; memcpy(&d, &bits, 4); return d; }
// the scene's device becomes the calling thread's current one, unless it is already
int use_device(const ctr_scene *s);
// a pointer of a query and the name its error messages give it
struct NamedPtr { const void *p; const char *name; };
// CTR_E_INVALID "<who><name> is not device memory of <whose>" for the first non-null pointer that is not memory of `device`
// (no size check is possible here): every pointer a kernel touches, for the ray queries (ctr_rays.cpp), the lens render's
// ray arrays and ctr_quantise_device's planes (ctr_render.cpp)
int check_device_pointers(int device, const std::string &who, const NamedPtr *ptrs, size_t n, const char *whose = "the scene's device");
template <size_t N>
int check_device_pointers(int device, const std::string &who, const NamedPtr (&ptrs)[N], const char *whose = "the scene's device") {
  return check_device_pointers(device, who, ptrs, N, whose);
}

// Memory the handle owns, in records of `elem` bytes: device memory, or page-locked host memory.  It only grows, and it is
// released with the handle (ctr_scene_destroy, the scene's device being current).  `tail`: bytes that stay readable behind the
// last record.
//   grow(n, keep)   room for `n` records.  Nothing happens when they fit; otherwise a new block of n * elem + tail bytes (never
//                   zero: n >= 1 here) receives the first `keep` records of the old one, copied where the memory lives (device
//                   to device: for a linear mesh the device's nodes are the unbounded payload, which the host copy does not
//                   hold), and only then is the old block freed and pointer and capacity set.  A failure leaves pointer, capacity
//                   and contents as they were.
//   reserve(n)      grow(n, 0): the contents may be gone afterwards.  For scratch.
struct GrowBuf {
  void *p = nullptr;
  size_t cap = 0;     // records
  size_t elem;        // bytes per record
  bool pinned;        // page-locked host memory instead of device memory
  size_t tail;        // bytes
  GrowBuf(size_t elem_bytes, bool pinned_host = false, size_t tail_bytes = 0) : elem(elem_bytes), pinned(pinned_host), tail(tail_bytes) {}
  GrowBuf(const GrowBuf &) = delete;
  ~GrowBuf() { release(); }
  int grow(size_t n, size_t keep);
  int reserve(size_t n) { return grow(n, 0); }
  void release();
  void swap(GrowBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }  // (two buffers of the same kind)
  template <class T> T *as() const { return (T *)p; }
};
// One of the scene's ten device arrays.  Each has 256 readable bytes behind its end: the leaf loop requests the three cache lines
// after a leaf's first triangle ahead of their use, whether the leaf has that many triangles or not (render_kernel.hip, "touch"),
// and the same kernels read the other nine.  The rule is stated HERE alone.
struct SceneBuf : GrowBuf {
  explicit SceneBuf(size_t rec) : GrowBuf(rec, false, 256) {}
};
// two buffers that grow as a pair: both hold `n` elements, or the next call tries again
inline int reserve_both(GrowBuf &a, GrowBuf &b, size_t n) { const int st = a.reserve(n); return st ? st : b.reserve(n); }

struct ctr_scene;
// the device receives the records a host-side edit changed (scene_flatten.h DirtyRange), in the order of the list
int upload_dirty(ctr_scene *s, const std::vector<DirtyRange> &dirty);
// The guard of the BVH culling: plan for the handle's cameras, lights and mirrors, apply to the host copy, upload what
// changed.  may_scan_on_device: the caller has waited for the device and allows the plane scan to run there (guard_scan.hip)
// when the scan is large enough to pay for a launch; false: the host scan, whatever its size.
int refresh_linear_meshes(ctr_scene *s, bool may_scan_on_device = false);
// ctr_scene_update_mesh: the planes of mesh guards[gi] changed, and src_dev is where the device holds the new ones already.  They
// replace the mesh's range of the scan's flat array by a copy on the device, if that array exists yet (the first scan on the
// device uploads every mesh from the host copy).
int guard_planes_changed(ctr_scene *s, size_t gi, const double *src_dev);
#pragma GCC visibility pop

// what ctr_scene_update_mesh keeps per mesh: the level schedule of its tree (mesh_refit.h) on the host and on the device
struct MeshRefit {
  LevelSchedule sched;
  GrowBuf d_nodes{sizeof(uint32_t)};  // sched.nodes, uploaded once
};

struct ctr_scene {
  int device = 0;
  FlatScene flat;             // the host copy of every scene array, and what the guard knows of it (scene_flatten.h)
  // the scene arrays on the device (ctr_scene.cpp scene_arrays: upload and partial re-upload); what a kernel sees of them is
  // made per call: device_scene() below.  Capacities are what ctr_scene_create allocated, until an edit needs more
  SceneBuf d_objs{sizeof(DObj)}, d_oloop{sizeof(DObj)}, d_meshes{sizeof(DObj)}, d_planes{sizeof(DPlanePair)}, d_tris{sizeof(DTri)};
  SceneBuf d_nodes{sizeof(DNode)}, d_nodes4{sizeof(DNode4)}, d_gnorm{4 * sizeof(float)}, d_lights{sizeof(DLight)}, d_mats{sizeof(DMat)};
  DCam cam{};                 // camera 0 (image size of every camera)
  GrowBuf d_cams{sizeof(DCam)};  // device camera array (>= 1 entry)
  uint32_t n_cams = 0;
  uint32_t cams_epoch = 0;    // bumped by ctr_scene_set_cameras / ctr_scene_set_size
  std::vector<DCam> h_cams;   // host copy of d_cams: the eyes the guard checks (refresh_linear_meshes)
  uint32_t user_variant = CTR_VAR_AUTO;
  bool no_scene_head = false;  // CUTRACE_NO_SCENE_HEAD=1 when the handle was created: launches carry an empty scene head
  bool no_shape_build = false; // CUTRACE_NO_SHAPE_BUILD=1 when the handle was created: every launch in shape KS_GENERAL (kernel_choice.h)
  bool no_wall_skip = false;   // CUTRACE_NO_WALL_SKIP=1 when the handle was created: every launch carries zero room facts (scene_device.h)
  bool no_dark_skip = false;   // CUTRACE_NO_DARK_SKIP=1 when the handle was created: every launch carries a zero dark-skip word (scene_device.h)
  bool no_opaque_build = false; // CUTRACE_NO_OPAQUE_BUILD=1 when the handle was created: no launch takes an opaque build (kernel_choice.h KO_*)
  bool no_phase_split = false;  // CUTRACE_NO_PHASE_SPLIT=1 when the handle was created: no launch takes a phased build (kernel_choice.h phased_build)
  struct RoomWords { float c[3], r, delta; uint32_t lights; } last_room{};  // the room facts of the most recent launch (ctr_debug_room_facts)
  uint32_t last_dark_skip = 0;  // its dark-skip word (ctr_debug_dark_skip)
  // cached device outputs for the host-buffer form: ONE allocation of 7 floats per pixel, a call's buffers are its
  // consecutive parts [depth px | color 3 px | normal 3 px] so that a frame can leave in a single D2H transfer
  GrowBuf out{7 * sizeof(float)};
  GrowBuf uv{2 * sizeof(float)};  // ctr_render_uv: 2 floats per pixel, allocated on first use
  GrowBuf img{9};                 // ctr_render_images: the three byte planes [depth8 | color8 | normal8], 9 bytes per pixel
  GrowBuf d_groups{sizeof(uint32_t)};        // host delivery: one completion counter per group of tiles (render_kernel.hip)
  GrowBuf h_groups{sizeof(uint32_t), true};  // page-locked landing zone of the counters (checked after every direct launch)
  GrowBuf h_counters{sizeof(unsigned long long), true};  // page-locked landing zone of the 16 counter words (first host-form render)
  unsigned long long last_cnt[16] = {0};     // the counter words of the last host-form render
  GrowBuf d_counters{sizeof(unsigned long long)};  // 16 words
  GrowBuf d_shards{sizeof(unsigned long long)};    // CTR_SHARDS x CTR_SHARD_WORDS, zero between launches
  uint32_t last_kernel = 0;        // the KV of the most recent launch (ctr_debug_last_kernel)
  uint32_t last_shape = 0;         // its launch shape, KS_* of kernel_choice.h (ctr_debug_last_shape)
  uint32_t last_opaque = 0;        // its opaque build, KO_* of kernel_choice.h (ctr_debug_last_opaque)
  uint32_t last_phased = 0;        // 1: it ran the phased twin of that opaque build (ctr_debug_last_phased)
  // tile scheduling feedback (include/cutrace_amd.h "Tile scheduling"; tile_order_policy.h, tile_order_host.cpp)
  OrderState order;
  GrowBuf d_cost{sizeof(uint32_t)}, d_order{sizeof(uint32_t)};  // order.cap tiles each
  bool poison_next_order = false;  // test hook (ctr_debug_poison_next_order)
  // mesh updates (include/cutrace_update.h, ctr_update.cpp): everything is allocated at the first update that needs it
  std::vector<std::unique_ptr<MeshRefit>> refit;  // one per FlatScene::guards entry; null until that mesh's first update
  GrowBuf upd_verts{sizeof(ctr_triangle)};         // a host input's vertices on the device
  GrowBuf upd_planes{7 * sizeof(double)};          // the guard's plane records as update_tris writes them
  GrowBuf upd_words{sizeof(uint32_t)};             // [0] the finiteness flag, [2..7] the mesh box
  GrowBuf upd_back{1, true};                       // page-locked landing zone of the copy-back, bytes
  // mesh rebuilds (include/cutrace_rebuild.h, ctr_update.cpp): the device builder's scratch (mesh_build.h), allocated at the first
  // rebuild; nothing of the scene lives in them
  GrowBuf rb_keys{sizeof(uint64_t)};               // 2 n: Morton keys, unsorted then sorted
  GrowBuf rb_index{sizeof(uint32_t)};              // 2 n: file indices, unsorted then sorted; afterwards [0, n) the accepted leaf order
  GrowBuf rb_temp{1};                              // the sort's temporary storage, bytes
  GrowBuf rb_bin{sizeof(LbvhNode)};                // the binary radix tree
  GrowBuf rb_nodes{sizeof(DNode4)};                // the collapsed descriptors, indexed by binary node
  GrowBuf rb_words{sizeof(float)};                 // [0..5] the centroid bounds, then the per-block partials
  // the guard's plane scan on the device (guard_scan.h, refresh_linear_meshes): everything is allocated at the first scan there
  GrowBuf scan_planes{7 * sizeof(double)};         // all meshes' planes, FlatScene::guards order
  bool scan_planes_live = false;                   // ... are on the device and current (false: the next scan uploads them all)
  GrowBuf scan_probes{sizeof(GuardProbe)};
  GrowBuf scan_words{sizeof(uint64_t)};            // one bit per plane
  GrowBuf scan_back{sizeof(uint64_t), true};       // page-locked landing zone of the words
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mtx;

  static uint64_t occ6_min_tris();  // CTR_OCC6_MIN_TRIS, or CUTRACE_OCC6_MIN_TRIS from the environment
  __attribute__((visibility("hidden"))) ~ctr_scene() = default;  // (releases every GrowBuf above; called by ctr_scene_destroy alone)
};

// the scene on the device as a launch or a query sees it now: the handle's arrays, the counts and flags of their host copy
inline DScene device_scene(const ctr_scene *s) {
  DScene D{};
  D.objs = s->d_objs.as<DObj>();
  D.oloop = s->d_oloop.as<DObj>();
  D.meshes = s->d_meshes.as<DObj>();
  D.planes = s->d_planes.as<DPlanePair>();
  D.tris = s->d_tris.as<DTri>();
  D.nodes = s->d_nodes.p;
  D.nodes4 = s->d_nodes4.p;
  D.gnorm = s->d_gnorm.as<float>();
  D.lights = s->d_lights.as<DLight>();
  D.mats = s->d_mats.as<DMat>();
  fill_scene_counts(s->flat, D);
  return D;
}

// An edit of the handle, from the first look at its host copy to the guard: the handle's lock is held while this lives.
//   begin()   before the first write: the scene's device is current and has been waited for, because no launch may still be
//             reading the old records.  Arguments are checked, and whatever can fail for want of memory is allocated, before
//             the first write to the handle.
//   end()     the device receives what the edit changed in the host copy, then the guard is refreshed (may_scan_on_device:
//             refresh_linear_meshes above)
struct Edit {
  ctr_scene *const s;
  std::lock_guard<std::mutex> lk;
  explicit Edit(ctr_scene *scene) : s(scene), lk(scene->mtx) {}
  int begin() const {
    if (int st = use_device(s)) return st;
    HIP_TRY(hipDeviceSynchronize());
    return CTR_OK;
  }
  int end(const std::vector<DirtyRange> &dirty, bool may_scan_on_device) const {
    if (int st = upload_dirty(s, dirty)) return st;
    return refresh_linear_meshes(s, may_scan_on_device);
  }
};

#endif
