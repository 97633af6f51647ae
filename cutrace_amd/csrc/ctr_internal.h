// ctr_internal.h — what the host translation units of the library share: the scene handle and the error / device helpers.
//
// Defined in ctr_api.cpp; used by ctr_api.cpp (the render path), ctr_rays.cpp (the ray queries) and ctr_multi.hip (the
// multi-device path).  Nothing here is part of the C-ABI.
#ifndef CUTRACE_AMD_CTR_INTERNAL_H
#define CUTRACE_AMD_CTR_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "cutrace_amd.h"
#include "scene_device.h"
#include "scene_flatten.h"

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

// is `p` page-locked host memory (hipHostMalloc / hipHostRegister)?  Then a D2H copy is one direct DMA.
bool is_pinned(const void *p);
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
// CTR_E_INVALID "<who><name> is not device memory of <whose>" for the first non-null pointer that is not memory of `device` (ctr_rays.cpp)
int check_device_pointers(int device, const std::string &who, const void *const *ptrs, const char *const *names, size_t n,
                          const char *whose = "the scene's device");
#pragma GCC visibility pop

struct ctr_scene {
  int device = 0;
  FlatScene flat;             // the host copy of every scene array below, and what the guard knows of it (scene_flatten.h)
  // the scene arrays on the device (ctr_api.cpp scene_arrays: upload, partial re-upload, free)
  DObj *d_objs = nullptr;
  DObj *d_oloop = nullptr;
  DObj *d_meshes = nullptr;
  DPlanePair *d_planes = nullptr;
  DTri *d_tris = nullptr;
  DNode *d_nodes = nullptr;
  DNode4 *d_nodes4 = nullptr;
  float *d_gnorm = nullptr;
  DLight *d_lights = nullptr;
  DMat *d_mats = nullptr;
  DCam cam{};                 // camera 0 (image size of every camera)
  DCam *d_cams = nullptr;     // device camera array (>= 1 entry)
  uint32_t n_cams = 0;
  uint32_t user_variant = CTR_VAR_AUTO;
  bool no_scene_head = false;  // CUTRACE_NO_SCENE_HEAD=1 when the handle was created: launches carry an empty scene head
  // cached device outputs for the host-buffer form: ONE allocation, a call's buffers are its consecutive
  // parts [depth px | color 3 px | normal 3 px] so that a frame can leave in a single D2H transfer
  float *d_out = nullptr;
  float *d_uv = nullptr;      // ctr_render_uv: 2 floats per pixel, allocated on first use
  size_t uv_px = 0;
  uint8_t *d_img = nullptr;   // ctr_render_images: the three byte planes [depth8 | color8 | normal8], 9 bytes per pixel, grown on use
  size_t img_px = 0;
  std::vector<DCam> h_cams;     // host copy of d_cams: the eyes the guard checks (refresh_linear_meshes)
  unsigned long long *h_counters = nullptr;  // pinned landing zone of the 16 counter words
  unsigned long long last_cnt[16] = {0};     // the counter words of the last host-form render
  unsigned long long *d_counters = nullptr;
  unsigned long long *d_shards = nullptr;  // CTR_SHARDS x CTR_SHARD_WORDS, zero between launches
  size_t out_px = 0;
  uint32_t *d_groups = nullptr;  // host delivery: one completion counter per group of tiles (render_kernel.hip)
  uint32_t *h_groups = nullptr;  // page-locked landing zone of the counters (checked after every direct launch)
  size_t groups_cap = 0;
  bool poison_next_order = false;  // test hook (ctr_debug_poison_next_order)
  uint32_t last_kernel = 0;        // the KV of the most recent launch (ctr_debug_last_kernel)
  // tile scheduling feedback (include/cutrace_amd.h "Tile scheduling"; tile_order.hip)
  uint32_t *d_cost = nullptr, *d_order = nullptr;
  uint32_t order_age = 0;  // launches of the current shape
  uint64_t order_view = 0; // camera set + first frame of the previous launch
  uint32_t cams_epoch = 0; // bumped by ctr_scene_set_cameras / ctr_scene_set_size
  size_t order_cap = 0;
  uint64_t order_key[6] = {0, 0, 0, 0, 0, 0};
  bool order_valid = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mtx;

  static uint64_t occ6_min_tris();  // CTR_OCC6_MIN_TRIS, or CUTRACE_OCC6_MIN_TRIS from the environment
};

#endif
