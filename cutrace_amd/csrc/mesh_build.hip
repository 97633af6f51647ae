// mesh_build.hip — the device builder of ctr_scene_rebuild_mesh (include/cutrace_rebuild.h; the host half is ctr_update.cpp): the
// SHAPE of a four-wide tree over one mesh's new vertices, as DNode4 descriptors.  The arithmetic is lbvh.h's, the text
// scripts/mesh_rebuild_check.cpp compiles for the host; boxes are not made here (mesh_update.hip refit_level makes them).
//
// Kernels of mesh_update.hip's shape: a lane owns what it writes, reads only the call's input and what an EARLIER launch on
// the same stream wrote, and ends.  No atomics, no waiting between workgroups: nothing here can spin.
//   centroid_partials  per-block min / max of the triangles' centroids (a wave reduces with shuffles, the block's four waves
//                      through 96 bytes of LDS), six floats per block
//   centroid_bounds    one block over the partials
//   morton_keys        one lane per triangle: (key, file index)
//   the sort           rocPRIM's radix_sort_pairs over the 63 key bits — plumbing; LSD and stable, so equal keys keep file order
//   radix_tree         one lane per internal node: Karras' construction
//   collapse           one lane per binary node: its DNode4 descriptors (sparse: indexed by binary node)
//   set_orig           the records' `orig` in the new leaf order
//
// Memory: 36 bytes read per triangle twice (bounds, keys), 12 per pair and pass of the sort, 128 written per binary node — a
// 64 000-triangle mesh moves ~20 MB, microseconds of HBM time next to the launches themselves.
#include <hip/hip_runtime.h>

#include <cstring>  // (before rocprim.hpp: its texture_cache_iterator.hpp calls memset without including it)
#include <rocprim/rocprim.hpp>

#include "lbvh.h"
#include "mesh_build.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t MB_THREADS = 256;
constexpr uint32_t MB_MAX_PARTIAL_BLOCKS = 1024;  // beyond that the lanes stride over the triangles

__device__ inline float wave_min(float x) {
  for (int off = 32; off >= 1; off >>= 1) x = fminf(x, __shfl_xor(x, off, 64));
  return x;
}
__device__ inline float wave_max(float x) {
  for (int off = 32; off >= 1; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// lo / hi of every lane of the block folded into out[0..5], by lane 0
__device__ inline void block_min_max(float *lo, float *hi, float *out) {
  __shared__ float part[MB_THREADS / 64][6];
  for (int a = 0; a < 3; a++) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
  const uint32_t wave = threadIdx.x / 64u;
  if (threadIdx.x % 64u == 0)
    for (int a = 0; a < 3; a++) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < MB_THREADS / 64; w++)
      for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], part[w][a]); hi[a] = fmaxf(hi[a], part[w][3 + a]); }
    for (int a = 0; a < 3; a++) { out[a] = lo[a]; out[3 + a] = hi[a]; }
  }
}

__global__ void __launch_bounds__(MB_THREADS) centroid_partials_kernel(const float *verts, uint32_t n, float *partials) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = blockIdx.x * MB_THREADS + threadIdx.x; t < n; t += gridDim.x * MB_THREADS) {
    float c[3];
    lbvh_centroid(verts, t, c);
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
  }
  block_min_max(lo, hi, partials + 6u * blockIdx.x);
}

__global__ void __launch_bounds__(MB_THREADS) centroid_bounds_kernel(const float *partials, uint32_t n_partials, float *bounds) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t b = threadIdx.x; b < n_partials; b += MB_THREADS)
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partials[6u * b + a]); hi[a] = fmaxf(hi[a], partials[6u * b + 3 + a]); }
  block_min_max(lo, hi, bounds);
}

__global__ void __launch_bounds__(MB_THREADS) morton_keys_kernel(const float *verts, uint32_t n, const float *bounds, uint64_t *keys, uint32_t *index) {
  const uint32_t t = blockIdx.x * MB_THREADS + threadIdx.x;
  if (t >= n) return;
  float c[3];
  lbvh_centroid(verts, t, c);
  keys[t] = lbvh_key(c, bounds, bounds + 3);
  index[t] = t;
}

__global__ void __launch_bounds__(MB_THREADS) radix_tree_kernel(const uint64_t *keys, uint32_t n, LbvhNode *bin) {
  const uint32_t i = blockIdx.x * MB_THREADS + threadIdx.x;
  if (i + 1u >= n) return;
  bin[i] = lbvh_node(keys, n, i);
}

__global__ void __launch_bounds__(MB_THREADS) collapse_kernel(const LbvhNode *bin, const uint64_t *keys, uint32_t n, uint32_t leaf, DNode4 *out) {
  const uint32_t i = blockIdx.x * MB_THREADS + threadIdx.x;
  if (i >= (n > 1u ? n - 1u : 1u)) return;
  lbvh_collapse(bin, keys, n, leaf, i, out);
}

__global__ void __launch_bounds__(MB_THREADS) set_orig_kernel(DTri *recs, const uint32_t *order, uint32_t n) {
  const uint32_t k = blockIdx.x * MB_THREADS + threadIdx.x;
  if (k < n) recs[k].orig = order[k];
}

uint32_t blocks_for(uint32_t lanes) { return (lanes + MB_THREADS - 1) / MB_THREADS; }
uint32_t partial_blocks(uint32_t n) { return std::min(blocks_for(n), MB_MAX_PARTIAL_BLOCKS); }

}  // namespace

size_t ctr_lbvh_partial_floats(uint32_t n) { return 6u * (size_t)std::max(partial_blocks(n), 1u); }

int ctr_launch_lbvh_bounds(const float *verts, uint32_t n, float *partials, float *bounds, void *stream) {
  if (n == 0) return 0;
  const uint32_t blocks = partial_blocks(n);
  hipLaunchKernelGGL(centroid_partials_kernel, dim3(blocks), dim3(MB_THREADS), 0, (hipStream_t)stream, verts, n, partials);
  if (hipError_t e = hipGetLastError()) return (int)e;
  hipLaunchKernelGGL(centroid_bounds_kernel, dim3(1), dim3(MB_THREADS), 0, (hipStream_t)stream, partials, blocks, bounds);
  return (int)hipGetLastError();
}

int ctr_launch_lbvh_keys(const float *verts, uint32_t n, const float *bounds, uint64_t *keys, uint32_t *index, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(morton_keys_kernel, dim3(blocks_for(n)), dim3(MB_THREADS), 0, (hipStream_t)stream, verts, n, bounds, keys, index);
  return (int)hipGetLastError();
}

int ctr_lbvh_sort_temp_bytes(uint32_t n, size_t *bytes) {
  *bytes = 0;
  return (int)rocprim::radix_sort_pairs(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                        (size_t)n, 0u, 3u * LBVH_AXIS_BITS, (hipStream_t) nullptr);
}

int ctr_lbvh_sort(void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *index_in, uint32_t *index_out,
                  uint32_t n, void *stream) {
  if (n == 0) return 0;
  return (int)rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, index_in, index_out, (size_t)n, 0u, 3u * LBVH_AXIS_BITS, (hipStream_t)stream);
}

int ctr_launch_lbvh_tree(const uint64_t *keys, uint32_t n, LbvhNode *bin, void *stream) {
  if (n < 2) return 0;
  hipLaunchKernelGGL(radix_tree_kernel, dim3(blocks_for(n - 1u)), dim3(MB_THREADS), 0, (hipStream_t)stream, keys, n, bin);
  return (int)hipGetLastError();
}

int ctr_launch_lbvh_collapse(const LbvhNode *bin, const uint64_t *keys, uint32_t n, uint32_t leaf, DNode4 *out, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(collapse_kernel, dim3(blocks_for(n > 1u ? n - 1u : 1u)), dim3(MB_THREADS), 0, (hipStream_t)stream, bin, keys, n, leaf, out);
  return (int)hipGetLastError();
}

int ctr_launch_set_orig(DTri *recs, const uint32_t *order, uint32_t n, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(set_orig_kernel, dim3(blocks_for(n)), dim3(MB_THREADS), 0, (hipStream_t)stream, recs, order, n);
  return (int)hipGetLastError();
}
