// ctr_multi.hip — one frame row-tiled over the GPUs of a node, ONE gather to device 0 (include/cutrace_amd.h).
//
// The reference is single-GPU (inc/kernel.hpp:86-130 launches one kernel on the current device); this is
// the multi-device form of the same boundary, SURVEY.md §8(b) item 3 / §8(e): the scene is tiny, so it is
// replicated on every device; pixels are independent, so device d renders the interleaved row blocks
// {b : b mod n == d} (contiguous bands are badly balanced; row_parts.h) into a compact buffer; the n-1 compact buffers
// travel to device 0 in ONE grouped RCCL send/recv over xGMI (7 messages on 7 distinct links at n = 8), a
// HIP kernel re-interleaves the row blocks into the row-major frame, and one D2H delivers it.
//
// Single process, one host thread, a render and a transfer stream per device — everything is asynchronous until the
// final synchronisation.  Built on the PUBLIC per-device entry points (ctr_scene_create, ctr_render_device), so
// a device's part is rendered by exactly the code the single-GPU path runs: results are bitwise those of
// ctr_render (tested).  RCCL (librccl.so, 570 MB) is dlopen'ed only when a group of >= 2 distinct devices
// is created; a group that lists one device several times (rehearsal on a one-GPU box) or a box without
// RCCL moves the parts with hipMemcpyPeerAsync instead.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "ctr_internal.h"
#include "cutrace_amd.h"
#include "row_parts.h"
#include "scene_device.h"

namespace {

// ---- RCCL, bound at run time ----
struct Rccl {
  void *lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  bool load() {
    if (lib) return true;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return false;
    CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
    GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
    Send = (decltype(Send))dlsym(lib, "ncclSend");
    Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
    GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
    return CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString;
  }
};
Rccl g_rccl;

// HIP_TRY under the name a step of the pipeline reports its HIP errors by
#define HIP_STEP(what, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return hip_fail(_e, what); } while (0)

constexpr int SLOTS = 2;  // frames in flight (ctr_multi_submit): frame k+1 renders while frame k is gathered and assembled

struct Slot {          // what one frame in flight needs of a part
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the render kernel (timing; ev1 = "rendered")
  hipEvent_t ev_moved = nullptr;   // the compact buffer has left / has been read: it may be rendered into again
  hipEvent_t ev_moved0 = nullptr;  // the same, recorded by DEVICE 0's transfer stream (peer copies; an event belongs to the device that records it)
  hipEvent_t ev_cnt = nullptr;     // the counters have landed on the host
  float *buf = nullptr;            // compact [depth px | color 3 px | normal 3 px] on the part's device
  unsigned long long *counters = nullptr;
  float *gathered = nullptr;       // the same bytes on device 0 (parts >= 1; part 0 only for "rccl-self")
};

struct Part {         // one device's share of the frame
  int device = 0;
  ctr_scene *scene = nullptr;
  hipStream_t stream = nullptr;          // render kernels of this device
  hipStream_t cstream = nullptr;         // this device's side of the gather (ncclSend); on device 0: receive, assemble, D2H
  Slot slot[SLOTS];
  uint64_t rows = 0;                     // rows of the current frame size this part owns
  ncclComm_t comm = nullptr;
};

// sources of the re-interleave: where part p's three compact buffers live on the assembling device
struct Reint {
  const float *depth[CTR_MULTI_MAX_DEVICES];
  const float *color[CTR_MULTI_MAX_DEVICES];
  const float *normal[CTR_MULTI_MAX_DEVICES];
  uint32_t n_parts, block_rows, w, h;
};

// Row y of the frame is local row k of part p:  p = (y / B) % n,  k = (y / B / n) * B + y % B.
// One workgroup copies one row of all three buffers (7 w floats), 16 bytes per lane where alignment allows.
__global__ __launch_bounds__(256) void reinterleave_rows(Reint R, float *__restrict__ out_depth, float *__restrict__ out_color,
                                                         float *__restrict__ out_normal) {
  const uint32_t y = blockIdx.x;
  const uint32_t blk = y / R.block_rows, p = blk % R.n_parts;
  const uint32_t k = (blk / R.n_parts) * R.block_rows + (y % R.block_rows);
  const float *src3[3] = {R.depth[p] + (size_t)k * R.w, R.color[p] + (size_t)k * R.w * 3, R.normal[p] + (size_t)k * R.w * 3};
  float *dst3[3] = {out_depth + (size_t)y * R.w, out_color + (size_t)y * R.w * 3, out_normal + (size_t)y * R.w * 3};
  const uint32_t len3[3] = {R.w, 3 * R.w, 3 * R.w};
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const float *a = src3[q];
    float *b = dst3[q];
    const uint32_t n = len3[q];
    if ((((uintptr_t)a | (uintptr_t)b) & 15u) == 0) {
      const uint32_t n4 = n / 4;
      for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) ((float4 *)b)[i] = ((const float4 *)a)[i];
      for (uint32_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) b[i] = a[i];
    } else {
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) b[i] = a[i];
    }
  }
}

// the one launch of reinterleave_rows: the parts' compact buffers become the row-major w x h frame `to`, on `stream`
hipError_t launch_reinterleave(const ctr_reint_part *parts, uint32_t n_parts, uint64_t block_rows, uint64_t w, uint64_t h,
                               const HostFrame &to, hipStream_t stream) {
  Reint R{{}, {}, {}, n_parts, (uint32_t)block_rows, (uint32_t)w, (uint32_t)h};
  for (uint32_t p = 0; p < n_parts; p++) {
    R.depth[p] = (const float *)parts[p].d_depth;
    R.color[p] = (const float *)parts[p].d_color3;
    R.normal[p] = (const float *)parts[p].d_normal3;
  }
  hipLaunchKernelGGL(reinterleave_rows, dim3((uint32_t)h), dim3(256), 0, stream, R, to.depth, to.color3, to.normal3);
  return hipGetLastError();
}

}  // namespace

struct Frame {         // one slot of the pipeline
  bool busy = false;
  bool sync_done = false;     // the frame went through ctr_render (one device, synchronous): nothing to wait for
  ctr_render_stats one{};     // ... and these are its statistics
  uint64_t h = 0;             // rows of the frame
  hipEvent_t ev_done = nullptr;   // device 0: the frame is assembled and on its way / in the caller's buffers
  std::chrono::high_resolution_clock::time_point t0;
};

struct ctr_multi {
  uint32_t variant = 0;
  double single_ms = -1.0;    // kernel ms of the last waited frame when it went through ctr_render (one device), else < 0
  std::vector<Part> parts;
  uint64_t w = 0, h = 0;
  uint64_t cap_px = 0;        // pixels each compact buffer can hold
  float *frame[SLOTS] = {};   // device 0: the re-interleaved frame [depth | color | normal]
  uint64_t frame_px = 0;
  unsigned long long *h_counters = nullptr;  // pinned, SLOTS x 16 words per part
  bool use_rccl = false;
  std::string transport = "single";
  Frame frames[SLOTS];
  int head = 0, inflight = 0;  // oldest frame in flight, number in flight
  int last = 0;                // slot of the frame waited for last (ctr_multi_kernel_ms)
};

namespace {

// ---- a part's streams and slots: on the part's device — but ev_moved0, which belongs to device 0 ----
int create_part(Part &P, int dev0) {
  HIP_TRY(hipSetDevice(dev0));
  for (Slot &S : P.slot) HIP_TRY(hipEventCreateWithFlags(&S.ev_moved0, hipEventDisableTiming));
  HIP_TRY(hipSetDevice(P.device));
  for (hipStream_t *s : {&P.stream, &P.cstream}) HIP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  for (Slot &S : P.slot) {
    for (hipEvent_t *e : {&S.ev0, &S.ev1}) HIP_TRY(hipEventCreate(e));
    for (hipEvent_t *e : {&S.ev_moved, &S.ev_cnt}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_TRY(hipMalloc((void **)&S.counters, 16 * sizeof(unsigned long long)));
  }
  return CTR_OK;
}

// whatever of a part exists goes (a part that create_part left half built included); nothing may be running on it
void release_part(Part &P, int dev0) {
  (void)hipSetDevice(P.device);
  if (P.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(P.comm);
  for (Slot &S : P.slot) {
    for (void *d : {(void *)S.buf, (void *)S.counters}) (void)hipFree(d);  // (null: nothing happens)
    for (hipEvent_t e : {S.ev0, S.ev1, S.ev_moved, S.ev_moved0, S.ev_cnt})
      if (e) (void)hipEventDestroy(e);
  }
  if (P.stream) (void)hipStreamDestroy(P.stream);
  if (P.cstream) (void)hipStreamDestroy(P.cstream);
  if (P.scene) ctr_scene_destroy(P.scene);
  (void)hipSetDevice(dev0);
  for (Slot &S : P.slot) (void)hipFree(S.gathered);
}

// both streams of every part have run dry: nothing is running on the group's buffers or into the caller's
void drain(ctr_multi *m) {
  for (Part &P : m->parts) {
    if (hipSetDevice(P.device) != hipSuccess) continue;
    if (P.stream) (void)hipStreamSynchronize(P.stream);
    if (P.cstream) (void)hipStreamSynchronize(P.cstream);
  }
}

// after an error: nothing may still be running on buffers the caller could free or reuse
int fail_sync(ctr_multi *m, int st) {
  drain(m);
  for (Frame &f : m->frames) f.busy = false;
  m->inflight = 0;
  (void)hipGetLastError();
  return st;
}

// How the parts will travel to device 0, decided once: "rccl" (distinct devices, unless CUTRACE_MULTI_TRANSPORT=peer), else
// "peer-copy".  One device and CUTRACE_MULTI_TRANSPORT=rccl-self: the self-test of the RCCL plumbing on a one-GPU box — a one-rank
// communicator, and the frame travels through the same grouped ncclSend / ncclRecv, to and from rank 0 itself.
void choose_transport(ctr_multi *m, const int *devices, int n_devices) {
  const char *force = getenv("CUTRACE_MULTI_TRANSPORT");
  bool distinct = true;
  for (int i = 0; i < n_devices; i++)
    for (int j = 0; j < i; j++)
      if (devices[i] == devices[j]) distinct = false;
  const bool self = n_devices == 1 && force && !strcmp(force, "rccl-self");
  if ((self || (n_devices > 1 && distinct && !(force && !strcmp(force, "peer")))) && g_rccl.load()) {
    std::vector<ncclComm_t> comms(n_devices);
    ncclResult_t r = g_rccl.CommInitAll(comms.data(), n_devices, devices);
    if (r == ncclSuccess) {
      for (int i = 0; i < n_devices; i++) m->parts[i].comm = comms[i];
      m->use_rccl = true;
      m->transport = self ? "rccl-self" : "rccl";
    } else {
      fail(CTR_E_HIP_BASE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r) + (self ? "" : " — falling back to peer copies"));
    }
  }
  if (n_devices == 1 || m->use_rccl) return;
  m->transport = "peer-copy";
  if (!distinct) return;
  (void)hipSetDevice(devices[0]);
  for (int i = 1; i < n_devices; i++) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) == hipSuccess && can && hipDeviceEnablePeerAccess(devices[i], 0) != hipSuccess)
      (void)hipGetLastError();  // already enabled is fine
  }
}

// ---- buffers that only grow ----
// *p is freed and, bytes != 0, allocated anew on `device`; a failure leaves it null
hipError_t renew(float *&p, int device, size_t bytes) {
  if (hipError_t e = hipSetDevice(device)) return e;
  (void)hipFree(p);
  p = nullptr;
  return bytes ? hipMalloc((void **)&p, bytes) : hipSuccess;
}

// Every part learns its rows of the frame at `block_rows`; the compact buffers hold the largest part, device 0's frames the
// whole image.  A capacity is zero while its buffers are renewed: an allocation that fails leaves null buffers, and the
// next call must come back here whatever its size.
int ensure_buffers(ctr_multi *m, uint64_t block_rows) {
  const uint32_t n = (uint32_t)m->parts.size();
  const int dev0 = m->parts[0].device;
  uint64_t cap = 1;
  for (uint32_t p = 0; p < n; p++) {
    m->parts[p].rows = part_rows(0, m->h, block_rows, p, n).n_rows;
    cap = cap > m->parts[p].rows * m->w ? cap : m->parts[p].rows * m->w;
  }
  const uint64_t frame_px = n > 1 ? m->w * m->h : 0;
  if (cap <= m->cap_px && frame_px <= m->frame_px) return CTR_OK;
  if (m->inflight) return fail(CTR_E_INVALID, "ctr_multi: the frame grew while frames are in flight (ctr_multi_wait first)");
  if (cap > m->cap_px) {
    m->cap_px = 0;
    for (uint32_t p = 0; p < n; p++)
      for (Slot &S : m->parts[p].slot) {
        HIP_TRY(renew(S.buf, m->parts[p].device, sizeof(float) * 7 * cap));
        // (part 0 has a gathered copy only under "rccl-self"; it is sized like everybody's and regrown with them —
        //  round 2 grew only the others', and a larger frame then overran it)
        HIP_TRY(renew(S.gathered, dev0, p > 0 || (n == 1 && m->use_rccl) ? sizeof(float) * 7 * cap : 0));
      }
    m->cap_px = cap;
  }
  if (frame_px > m->frame_px) {
    m->frame_px = 0;
    for (float *&fr : m->frame) HIP_TRY(renew(fr, dev0, sizeof(float) * 7 * frame_px));
    m->frame_px = frame_px;
  }
  return CTR_OK;
}

// ---- the steps of ctr_multi_submit, in the order it takes them ----
struct Job {  // one frame being queued: its slot, what to render, whereto
  int q, bounces;
  float fudge;
  uint64_t block_rows;
  HostFrame out, z;          // the caller's buffers; direct: the same buffers as device 0 sees them
  bool direct, dest_pinned;  // device 0's kernels write the caller's buffers themselves; all three are page-locked
};

// Page-locked destinations are written by device 0 itself: through ctr_render's host delivery when there is one
// device, by the re-interleave kernel (whole rows, 16 bytes per lane) otherwise — no frame-sized D2H after it.
// (CTR_VAR_NO_DIRECT is asked before any pointer is looked at.)
int pick_destination(ctr_multi *m, Job &J) {
  const Part &P0 = m->parts[0];
  HIP_TRY(hipSetDevice(P0.device));
  J.direct = !(m->variant & CTR_VAR_NO_DIRECT) && device_visible(J.out, m->w * m->h, J.z);
  J.dest_pinned = J.direct || all_pinned(J.out, m->w * m->h);
  return CTR_OK;
}

// One device: ctr_render is the better path both for page-locked destinations (delivered by the kernel) and for
// pageable ones (its three plain copies: 2.2 ms per 1080p frame where queuing them on a side stream took 4.8).
// An earlier frame may have taken the asynchronous path (a page-locked destination under CTR_VAR_NO_DIRECT) and still
// be running on P0's streams, which do not synchronise with the null stream ctr_render launches on: two launches on
// ONE scene handle would share its counter shards, cost table and dispatch order.  Drain it first; the
// frame stays queued (its events have fired by then, ctr_multi_wait returns it at once).
int render_synchronously(ctr_multi *m, const Job &J, Frame &F) {
  Part &P0 = m->parts[0];
  if (m->inflight)
    for (hipStream_t s : {P0.stream, P0.cstream}) HIP_STEP("ctr_multi_submit", hipStreamSynchronize(s));
  if (int st = ctr_render(P0.scene, J.fudge, J.bounces, nullptr, J.out.depth, J.out.color3, J.out.normal3, &F.one)) return st;
  F.sync_done = true;
  return CTR_OK;
}

// every device renders its interleaved row blocks into its compact buffer of the slot, on its render stream
int render_parts(ctr_multi *m, const Job &J) {
  const uint32_t n = (uint32_t)m->parts.size();
  unsigned long long *hc = m->h_counters + (size_t)16 * n * J.q;
  for (uint32_t p = 0; p < n; p++) {
    Part &P = m->parts[p];
    Slot &S = P.slot[J.q];
    HIP_STEP("hipSetDevice", hipSetDevice(P.device));
    HIP_STEP("ctr_multi_submit", hipStreamWaitEvent(P.stream, S.ev_moved, 0));  // (never recorded yet: no wait)
    HIP_STEP("ctr_multi_submit", hipStreamWaitEvent(P.stream, S.ev_moved0, 0));
    HIP_STEP("ctr_multi_submit", hipMemsetAsync(S.counters, 0, 16 * sizeof(unsigned long long), P.stream));
    HIP_STEP("ctr_multi_submit", hipEventRecord(S.ev0, P.stream));
    const uint64_t px = P.rows * m->w;
    const ctr_rows r{0, m->h, J.block_rows, p, n};
    if (int st = px ? ctr_render_device(P.scene, J.fudge, J.bounces, &r, S.buf, S.buf + px, S.buf + 4 * px, S.counters, P.stream) : CTR_OK) return st;
    HIP_STEP("ctr_multi_submit", hipEventRecord(S.ev1, P.stream));
    HIP_STEP("ctr_multi_submit", hipMemcpyAsync(hc + 16 * p, S.counters, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, P.stream));
    HIP_STEP("ctr_multi_submit", hipEventRecord(S.ev_cnt, P.stream));
  }
  return CTR_OK;
}

// The RCCL gather: the compact buffers of parts first .. n-1 travel to rank 0 in ONE grouped send / receive, each on its
// device's transfer stream, the receives on device 0's.  first = 1 for a group of n devices; first = 0 is "rccl-self",
// where rank 0 sends its own part to itself: the same calls, one rank.
int rccl_gather(ctr_multi *m, int q, uint32_t first) {
  const uint32_t n = (uint32_t)m->parts.size();
  Part &P0 = m->parts[0];
  for (uint32_t p = first; p < n; p++) {  // a device sends once its own kernel is done
    HIP_STEP("RCCL gather", hipSetDevice(m->parts[p].device));
    HIP_STEP("RCCL gather", hipStreamWaitEvent(m->parts[p].cstream, m->parts[p].slot[q].ev1, 0));
  }
  // (no early return between GroupStart and GroupEnd: an open group would poison every later call)
  hipError_t he = hipSuccess;
  ncclResult_t r = g_rccl.GroupStart();
  for (uint32_t p = first; p < n && r == ncclSuccess && he == hipSuccess; p++) {
    Part &P = m->parts[p];
    const size_t cnt = (size_t)(7 * P.rows * m->w);
    if (!cnt) continue;
    if ((he = hipSetDevice(P.device)) != hipSuccess) break;
    if ((r = g_rccl.Send(P.slot[q].buf, cnt, ncclFloat, 0, P.comm, P.cstream)) != ncclSuccess) break;
    if ((he = hipSetDevice(P0.device)) != hipSuccess) break;
    r = g_rccl.Recv(P.slot[q].gathered, cnt, ncclFloat, (int)p, P0.comm, P0.cstream);
  }
  const ncclResult_t r2 = g_rccl.GroupEnd();
  if (r == ncclSuccess) r = r2;
  if (he != hipSuccess) return hip_fail(he, "RCCL gather");
  if (r != ncclSuccess) return fail(CTR_E_HIP_BASE, std::string(first ? "RCCL gather: " : "RCCL self send/recv: ") + g_rccl.GetErrorString(r));
  // sent: the compact buffer may be rendered into again (but part 0's, still to be read on device 0: queue_frame)
  for (uint32_t p = 1; p < n; p++) {
    HIP_STEP("gather", hipSetDevice(m->parts[p].device));
    HIP_STEP("gather", hipEventRecord(m->parts[p].slot[q].ev_moved, m->parts[p].cstream));
  }
  return CTR_OK;
}

// the same gather without RCCL: device 0's transfer stream fetches every other part once that part is rendered
int peer_gather(ctr_multi *m, int q) {
  Part &P0 = m->parts[0];
  HIP_STEP("gather", hipSetDevice(P0.device));
  for (uint32_t p = 1; p < m->parts.size(); p++) {
    Part &P = m->parts[p];
    Slot &S = P.slot[q];
    const size_t bytes = sizeof(float) * 7 * P.rows * m->w;
    HIP_STEP("gather", hipStreamWaitEvent(P0.cstream, S.ev1, 0));
    if (bytes && P.device == P0.device) HIP_STEP("gather", hipMemcpyAsync(S.gathered, S.buf, bytes, hipMemcpyDeviceToDevice, P0.cstream));
    else if (bytes) HIP_STEP("gather", hipMemcpyPeerAsync(S.gathered, P0.device, S.buf, P.device, bytes, P0.cstream));
    HIP_STEP("gather", hipEventRecord(S.ev_moved0, P0.cstream));
  }
  return CTR_OK;
}

// one gather to device 0, on the transfer streams; it leaves device 0 current
int gather(ctr_multi *m, int q) {
  Part &P0 = m->parts[0];
  const bool self = m->parts.size() == 1 && m->use_rccl;  // "rccl-self": the frame goes through RCCL once, rank 0 -> rank 0
  const int st = m->use_rccl ? rccl_gather(m, q, self ? 0 : 1) : m->parts.size() > 1 ? peer_gather(m, q) : CTR_OK;
  if (st || self) return st;  // (as a sender, rank 0 has waited for its kernel already)
  // Device 0's transfer stream also needs device 0's own part — asked for AFTER the receives are queued: before them, the
  // whole gather would stand behind device 0's kernel.
  HIP_STEP("ctr_multi_submit", hipSetDevice(P0.device));
  HIP_STEP("ctr_multi_submit", hipStreamWaitEvent(P0.cstream, P0.slot[q].ev1, 0));
  return CTR_OK;
}

// Device 0 re-interleaves the parts into the row-major frame: the caller's buffers (direct) or the slot's frame buffer.
// *result: where copy_out finds the frame.  One part: its compact buffer IS the frame ("rccl-self": its copy that went through RCCL).
int assemble(ctr_multi *m, const Job &J, const float **result) {
  const uint32_t n = (uint32_t)m->parts.size();
  const Part &P0 = m->parts[0];
  const uint64_t w = m->w, fpx = m->w * m->h;
  float *fr = m->frame[J.q];
  *result = n > 1 ? fr : m->use_rccl ? P0.slot[J.q].gathered : P0.slot[J.q].buf;
  if (n == 1 || !fpx) return CTR_OK;
  ctr_reint_part src[CTR_MULTI_MAX_DEVICES];
  for (uint32_t p = 0; p < n; p++) {
    const float *s = p == 0 ? P0.slot[J.q].buf : m->parts[p].slot[J.q].gathered;
    const size_t px = (size_t)(m->parts[p].rows * w);
    src[p] = {s, s + px, s + 4 * px};
  }
  const HostFrame to = J.direct ? J.z : HostFrame{fr, fr + fpx, fr + 4 * fpx, nullptr};
  HIP_STEP("reinterleave_rows", launch_reinterleave(src, n, J.block_rows, w, m->h, to, P0.cstream));
  return CTR_OK;
}

// The frame leaves device 0 on its transfer stream, unless the re-interleave kernel wrote the caller's buffers itself: in
// one D2H where the destination is one packed page-locked block, else one per buffer.
int copy_out(ctr_multi *m, const Job &J, const float *result) {
  const uint64_t fpx = m->w * m->h;
  const HostFrame &o = J.out;
  hipStream_t cs = m->parts[0].cstream;
  if (!fpx || (J.direct && m->parts.size() > 1)) return CTR_OK;
  const bool one = J.dest_pinned && o.depth && o.color3 == o.depth + fpx && o.normal3 == o.color3 + 3 * fpx;
  // (hipMemcpyAsync into pageable memory is staged by the runtime and returns when the copy is done)
  if (o.depth) HIP_STEP("frame copy-out", hipMemcpyAsync(o.depth, result, sizeof(float) * (one ? 7 : 1) * fpx, hipMemcpyDeviceToHost, cs));
  if (o.color3 && !one) HIP_STEP("frame copy-out", hipMemcpyAsync(o.color3, result + fpx, sizeof(float) * 3 * fpx, hipMemcpyDeviceToHost, cs));
  if (o.normal3 && !one) HIP_STEP("frame copy-out", hipMemcpyAsync(o.normal3, result + 4 * fpx, sizeof(float) * 3 * fpx, hipMemcpyDeviceToHost, cs));
  return CTR_OK;
}

// One frame is queued, step by step; a step that fails ends it (ctr_multi_submit then drains the streams).
int queue_frame(ctr_multi *m, Job &J, Frame &F) {
  Part &P0 = m->parts[0];
  int st = pick_destination(m, J);
  if (st) return st;
  if (m->parts.size() == 1 && !m->use_rccl && (J.direct || !J.dest_pinned)) return render_synchronously(m, J, F);
  const float *result = nullptr;
  if ((st = render_parts(m, J)) || (st = gather(m, J.q)) || (st = assemble(m, J, &result)) || (st = copy_out(m, J, result))) return st;
  // device 0's compact buffer has been read once the assembly (or, one part, the copy-out) is through
  HIP_STEP("ctr_multi_submit", hipEventRecord(P0.slot[J.q].ev_moved, P0.cstream));
  HIP_STEP("ctr_multi_submit", hipEventRecord(F.ev_done, P0.cstream));
  return CTR_OK;
}

// ctr_multi_wait past its checks: the frame of slot q is in the caller's buffers, its counters are on the host and every
// compact buffer has been read; stats: kernel_ms = the slowest device's kernel, ray_count = sum, max_depth = max
int finish_slot(ctr_multi *m, int q, ctr_render_stats *stats) {
  HIP_STEP("ctr_multi_wait", hipSetDevice(m->parts[0].device));
  HIP_STEP("ctr_multi_wait", hipEventSynchronize(m->frames[q].ev_done));
  for (Part &P : m->parts) {
    HIP_STEP("ctr_multi_wait", hipSetDevice(P.device));
    for (hipEvent_t e : {P.slot[q].ev_cnt, P.slot[q].ev_moved, P.slot[q].ev_moved0}) HIP_STEP("ctr_multi_wait", hipEventSynchronize(e));
  }
  if (!stats) return CTR_OK;
  const auto t1 = std::chrono::high_resolution_clock::now();
  const unsigned long long *cnt = m->h_counters + (size_t)16 * m->parts.size() * q;  // 16 words per part
  uint32_t deepest = 0;  // (the bit patterns of floats >= 0 order like the floats)
  memset(stats, 0, sizeof(*stats));
  for (const Part &P : m->parts) {
    float ms = 0.f;
    HIP_TRY(hipSetDevice(P.device));
    HIP_TRY(hipEventElapsedTime(&ms, P.slot[q].ev0, P.slot[q].ev1));
    stats->kernel_ms = stats->kernel_ms > ms ? stats->kernel_ms : ms;
    stats->ray_count += cnt[0];
    deepest = deepest > (uint32_t)cnt[1] ? deepest : (uint32_t)cnt[1];
    cnt += 16;
  }
  stats->max_depth = depth_of_counter(deepest);
  stats->rows = m->frames[q].h;
  stats->total_ms = std::chrono::duration<double, std::milli>(t1 - m->frames[q].t0).count();
  return CTR_OK;
}

}  // namespace

extern "C" {

int ctr_multi_create(const ctr_scene_desc *desc, const int *devices, int n_devices, ctr_multi **out) {
  if (!desc || !devices || !out || n_devices < 1 || n_devices > CTR_MULTI_MAX_DEVICES)
    return fail(CTR_E_INVALID, "ctr_multi_create: bad argument (1.." + std::to_string(CTR_MULTI_MAX_DEVICES) + " devices)");
  *out = nullptr;
  std::unique_ptr<ctr_multi, void (*)(ctr_multi *)> group(new ctr_multi(), ctr_multi_destroy);  // destroyed on every early return
  ctr_multi *m = group.get();
  m->w = desc->cam.w;
  m->h = desc->cam.h;
  m->parts.resize(n_devices);
  for (int i = 0; i < n_devices; i++) m->parts[i].device = devices[i];
  for (Part &P : m->parts) {
    if (int st = ctr_scene_create(desc, P.device, &P.scene)) return st;  // the scene is replicated: it is < 1 MB
    if (int st = create_part(P, devices[0])) return st;
  }
  HIP_TRY(hipHostMalloc((void **)&m->h_counters, sizeof(unsigned long long) * 16 * n_devices * SLOTS, hipHostMallocDefault));
  HIP_TRY(hipSetDevice(devices[0]));
  for (Frame &F : m->frames) HIP_TRY(hipEventCreateWithFlags(&F.ev_done, hipEventDisableTiming));
  choose_transport(m, devices, n_devices);
  *out = group.release();
  return CTR_OK;
}

void ctr_multi_destroy(ctr_multi *m) {
  if (!m) return;
  drain(m);  // nothing may be running when the buffers go
  const int dev0 = m->parts.empty() ? 0 : m->parts[0].device;
  for (Part &P : m->parts) release_part(P, dev0);
  for (int q = 0; q < SLOTS; q++) {
    if (m->frame[q]) (void)hipFree(m->frame[q]);
    if (m->frames[q].ev_done) (void)hipEventDestroy(m->frames[q].ev_done);
  }
  if (m->h_counters) (void)hipHostFree(m->h_counters);
  delete m;
}

int ctr_multi_devices(const ctr_multi *m) { return m ? (int)m->parts.size() : 0; }
const char *ctr_multi_transport(const ctr_multi *m) { return m ? m->transport.c_str() : ""; }

int ctr_multi_size(const ctr_multi *m, uint64_t *w, uint64_t *h) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  if (w) *w = m->w;
  if (h) *h = m->h;
  return CTR_OK;
}

int ctr_multi_set_size(ctr_multi *m, uint64_t w, uint64_t h) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  if (m->inflight) return fail(CTR_E_INVALID, "ctr_multi_set_size: frames in flight (ctr_multi_wait first)");
  for (Part &P : m->parts)
    if (int st = ctr_scene_set_size(P.scene, w, h)) return st;
  m->w = w;
  m->h = h;
  return CTR_OK;
}

int ctr_multi_set_variant(ctr_multi *m, uint32_t bits) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  for (Part &P : m->parts)
    if (int st = ctr_set_variant(P.scene, bits)) return st;
  m->variant = bits;
  return CTR_OK;
}

// ---- the pipeline ----
// ctr_multi_submit queues one frame and returns; ctr_multi_wait returns when the OLDEST queued frame is in the caller's
// buffers.  Two frames may be in flight, each in its own slot of every buffer.  Per device a render stream and a
// transfer stream: the kernel of frame k+1 starts as soon as that of frame k is done, while frame k's compact buffers
// travel to device 0 (one grouped ncclSend / ncclRecv), are re-interleaved there and leave for the host.  What orders them:
//   ev1       rendered      -> the device's send / device 0's assembly may read the compact buffer
//   ev_moved  sent / read   -> the render stream may write the compact buffer again (frame k+2)
//   ev_done   assembled, copied out -> ctr_multi_wait
// ctr_render_multi = submit + wait.  One device with a page-locked or pageable destination goes through ctr_render
// (host delivery / its own copies) and is synchronous; "page-locked" is what makes the final D2H asynchronous at all.
// queue_frame takes the steps; whichever of them fails, the streams are drained and the queue is emptied (fail_sync).
int ctr_multi_submit(ctr_multi *m, float fudge, int bounces, uint64_t block_rows, float *depth, float *color3, float *normal3) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  if (m->inflight >= SLOTS) return fail(CTR_E_INVALID, "ctr_multi_submit: two frames are in flight already (ctr_multi_wait first)");
  if (block_rows == 0) block_rows = 8;
  if (int st = ensure_buffers(m, block_rows)) return st;
  Job J{(m->head + m->inflight) % SLOTS, bounces, fudge, block_rows, HostFrame{depth, color3, normal3, nullptr}, HostFrame{}, false, false};
  Frame &F = m->frames[J.q];
  F.t0 = std::chrono::high_resolution_clock::now();
  F.sync_done = false;
  F.h = m->h;
  if (int st = queue_frame(m, J, F)) return fail_sync(m, st);
  F.busy = true;
  m->inflight++;
  return CTR_OK;
}

int ctr_multi_wait(ctr_multi *m, ctr_render_stats *stats) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  if (m->inflight == 0) return fail(CTR_E_INVALID, "ctr_multi_wait: no frame in flight");
  const int q = m->head;
  Frame &F = m->frames[q];
  m->single_ms = -1.0;
  if (F.sync_done) {
    m->single_ms = F.one.kernel_ms;
    if (stats) {
      *stats = F.one;
      stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - F.t0).count();
    }
  } else {
    if (int st = finish_slot(m, q, stats)) return fail_sync(m, st);
  }
  F.busy = false;
  m->last = q;
  m->head = (m->head + 1) % SLOTS;
  m->inflight--;
  return CTR_OK;
}

int ctr_render_multi(ctr_multi *m, float fudge, int bounces, uint64_t block_rows, float *depth, float *color3,
                     float *normal3, ctr_render_stats *stats) {
  if (!m) return fail(CTR_E_INVALID, "null group");
  if (m->inflight) return fail(CTR_E_INVALID, "ctr_render_multi: frames are in flight (ctr_multi_wait first)");
  if (int st = ctr_multi_submit(m, fudge, bounces, block_rows, depth, color3, normal3)) return st;
  return ctr_multi_wait(m, stats);
}

int ctr_reinterleave_device(const ctr_reint_part *parts, uint32_t n_parts, uint64_t block_rows, uint64_t w, uint64_t h,
                            void *d_depth, void *d_color3, void *d_normal3, void *hip_stream) {
  if (!parts || n_parts == 0 || n_parts > CTR_MULTI_MAX_DEVICES || block_rows == 0 || !d_depth || !d_color3 || !d_normal3)
    return fail(CTR_E_INVALID, "ctr_reinterleave_device: bad argument");
  if (w == 0 || h == 0) return CTR_OK;
  if (w > 0x7FFFFFFFull || h > 0x7FFFFFFFull) return fail(CTR_E_INVALID, "ctr_reinterleave_device: image too large");
  const HostFrame to{(float *)d_depth, (float *)d_color3, (float *)d_normal3, nullptr};
  HIP_STEP("hipGetLastError()", launch_reinterleave(parts, n_parts, block_rows, w, h, to, (hipStream_t)hip_stream));
  return CTR_OK;
}

int ctr_multi_kernel_ms(ctr_multi *m, double *ms_per_device, int capacity) {
  if (!m || !ms_per_device) return fail(CTR_E_INVALID, "ctr_multi_kernel_ms: null argument");
  if (m->single_ms >= 0.0 && capacity > 0) {
    ms_per_device[0] = m->single_ms;
    return CTR_OK;
  }
  for (int p = 0; p < (int)m->parts.size() && p < capacity; p++) {
    float ms = 0.f;
    HIP_TRY(hipSetDevice(m->parts[p].device));
    HIP_TRY(hipEventElapsedTime(&ms, m->parts[p].slot[m->last].ev0, m->parts[p].slot[m->last].ev1));
    ms_per_device[p] = ms;
  }
  return CTR_OK;
}

}  // extern "C"
