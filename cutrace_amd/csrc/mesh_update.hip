// mesh_update.hip — the device half of ctr_scene_update_mesh (include/cutrace_update.h; the host half is ctr_update.cpp): new
// vertices of one mesh become its DTri records, normals and guard planes, and the boxes of its tree are refitted.
//
// Four small kernels, all of one shape: a lane owns what it writes, reads only the call's input and what an EARLIER launch
// on the same stream wrote, and ends.  No LDS, no atomics, no waiting between workgroups: nothing here can spin.
//   all_finite   one flag word, set with a plain vector store by every lane that meets a NaN or an infinity (they all
//                store the same 1, so the race between them is harmless)
//   update_tris  one lane per leaf-order record: tri_record.h, the text scene_flatten.cpp compiles for the host
//   refit_level  one lane per (node, slot) of one height level: mesh_refit.h; one launch per level, lowest first
//   mesh_box     six floats from the refitted root
//
// Numerics: the library's -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt (build.py HIP_FLAGS) make every f32
// and f64 operation of tri_record.h the correctly rounded one the host performs; the pragma below keeps contraction off
// under the compiler's default as well.
//
// Memory: update_tris reads 40 bytes and writes 136 per triangle, refit_level moves a few hundred bytes per node; a
// 64 000-triangle mesh is ~11 MB in all, microseconds of HBM time.  The DTri record leaves as four 16-byte stores per lane
// (a wave covers 4 KiB contiguously), the normal as one; the reads through `orig` are a gather and stay 4-byte loads.
#include <hip/hip_runtime.h>

#include "mesh_refit.h"
#include "mesh_update.h"
#include "tri_record.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t MU_THREADS = 256;
constexpr uint64_t MU_MAX_BLOCKS = 1u << 16;  // all_finite: beyond that the lanes stride over the input

__global__ void __launch_bounds__(MU_THREADS) all_finite_kernel(const float *v, uint64_t n, uint32_t *flag) {
  const uint64_t stride = (uint64_t)gridDim.x * MU_THREADS;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * MU_THREADS + threadIdx.x; i < n; i += stride) bad |= !__builtin_isfinite(v[i]);
  if (bad) *flag = 1u;
}

__global__ void __launch_bounds__(MU_THREADS) update_tris_kernel(DTri *recs, float *gn, double *planes, const float *verts, uint32_t n) {
  const uint32_t k = blockIdx.x * MU_THREADS + threadIdx.x;
  if (k >= n) return;
  const uint32_t orig = recs[k].orig;
  const float *v = verts + 9u * (size_t)orig;
  const ctr_vec3 p1{v[0], v[1], v[2]}, p2{v[3], v[4], v[5]}, p3{v[6], v[7], v[8]};
  DTri T;
  float g[4];
  make_tri(p1, p2, p3, orig, T, g);
  float4 *out = reinterpret_cast<float4 *>(recs + k);  // 64-byte records of a hipMalloc'ed array: 16-byte aligned
  out[0] = make_float4(T.ab[0][0], T.ab[0][1], T.ab[1][0], T.ab[1][1]);
  out[1] = make_float4(T.ab[2][0], T.ab[2][1], T.px, T.py);
  out[2] = make_float4(T.pz, __uint_as_float(T.orig), T.nx, T.ny);
  out[3] = make_float4(T.nz, T.ke, T.ke2, T.pad1);
  *reinterpret_cast<float4 *>(gn + 4u * (size_t)orig) = make_float4(g[0], g[1], g[2], g[3]);  // normals in FILE order
  double q[CTR_PLANE_DOUBLES];
  guard_plane(p1, p2, p3, q);
  double *pl = planes + (size_t)CTR_PLANE_DOUBLES * k;
  for (int j = 0; j < CTR_PLANE_DOUBLES; j++) pl[j] = q[j];
}

__global__ void __launch_bounds__(MU_THREADS) refit_level_kernel(DNode4 *nodes, const uint32_t *sched, uint32_t n_nodes, const DTri *recs,
                                                                 const float *verts) {
  const uint32_t i = blockIdx.x * MU_THREADS + threadIdx.x;
  if (i >= 4u * n_nodes) return;
  refit_slot(nodes, sched[i >> 2], (int)(i & 3u), recs, verts);
}

__global__ void __launch_bounds__(64) mesh_box_kernel(const DNode4 *nodes, float *box) {
  if (threadIdx.x != 0) return;
  float b[6];
  refit_mesh_box(nodes[0], b);
  for (int j = 0; j < 6; j++) box[j] = b[j];
}

}  // namespace

int ctr_launch_all_finite(const float *v, uint64_t n, uint32_t *flag, void *stream) {
  if (n == 0) return 0;
  const uint64_t blocks = (n + MU_THREADS - 1) / MU_THREADS;
  const dim3 grid((uint32_t)(blocks < MU_MAX_BLOCKS ? blocks : MU_MAX_BLOCKS));
  hipLaunchKernelGGL(all_finite_kernel, grid, dim3(MU_THREADS), 0, (hipStream_t)stream, v, n, flag);
  return (int)hipGetLastError();
}

int ctr_launch_update_tris(DTri *recs, float *gn, double *planes, const float *verts, uint32_t n, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(update_tris_kernel, dim3((n + MU_THREADS - 1) / MU_THREADS), dim3(MU_THREADS), 0, (hipStream_t)stream, recs, gn, planes,
                     verts, n);
  return (int)hipGetLastError();
}

int ctr_launch_refit_level(DNode4 *nodes, const uint32_t *sched, uint32_t n_nodes, const DTri *recs, const float *verts, void *stream) {
  if (n_nodes == 0) return 0;
  hipLaunchKernelGGL(refit_level_kernel, dim3((4u * n_nodes + MU_THREADS - 1) / MU_THREADS), dim3(MU_THREADS), 0, (hipStream_t)stream, nodes,
                     sched, n_nodes, recs, verts);
  return (int)hipGetLastError();
}

int ctr_launch_mesh_box(const DNode4 *nodes, float *box, void *stream) {
  hipLaunchKernelGGL(mesh_box_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, nodes, box);
  return (int)hipGetLastError();
}
