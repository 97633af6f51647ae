// tile_order.hip — the tile scheduler: in which order the render kernel's waves take the tiles of a launch.
//
// Waves differ 10x in cost and the hardware hands them out in blockIdx order, so with tiles in image order the last
// quarter of a frame is a tail of a few slow waves on an otherwise empty GPU.  The render kernel (render_kernel.hip
// "Dispatch order") takes its tile from an order buffer and records what the tile cost; two small kernels around it, on
// the same stream, make that buffer:
//  * after_render: tiles are dispatched expensive-first from the costs the previous launch recorded, which removes the
//    tail of slow waves at the end of a frame (a counting sort by cost class; for "Host delivery" launches over groups of
//    tiles, so that a group completes soon after its first tile starts).  The same kernel folds the counter shards the
//    render kernel added into.
//  * first_order: a shape nothing is known about yet is dispatched centre-out.
// Any permutation of the tiles is a correct order: the order only shapes the tail of a launch, never a pixel.
//
// Also here, because it follows from the same tile shape (tile_shape.h): the host's view of the launch's tile and
// staging geometry (ctr_launch_waves, ctr_staging_*, ctr_group_tile_count).  Nothing in this file shares code or
// registers with the render kernel.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "scene_device.h"
#include "tile_order.h"
#include "tile_shape.h"

// counters of the counting sort (64 cost classes x 16 sub-bins) = threads of its block
#define CTR_COST_BINS 1024u
#ifndef CTR_CHEAP_FIRST_PCT
#define CTR_CHEAP_FIRST_PCT 25u  // order_block_groups: share of the groups, the cheapest, dispatched before the dear ones
#endif

namespace {

// ---- after_render: block 0 folds the counter shards, block 1 builds the next dispatch order ----
// block of CTR_SHARDS threads: thread t owns shard t; wave-level reduction, then one LDS atomic per
// wave and word; adds into out[0..14] (max for word 1) and zeroes the shards for the next launch
__device__ void fold_block(unsigned long long *__restrict__ shards, unsigned long long *__restrict__ out) {
  constexpr int NW = 15;
  __shared__ unsigned long long acc[NW];
  if (threadIdx.x < NW) acc[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long *sh = shards + (size_t)threadIdx.x * CTR_SHARD_WORDS;
  unsigned long long v[NW];
#pragma unroll
  for (int q = 0; q < NW; q++) {
    v[q] = sh[q];
    if (v[q]) sh[q] = 0ull;
  }
#pragma unroll
  for (int q = 0; q < NW; q++) {
    unsigned long long x = v[q];
    if (__builtin_amdgcn_ballot_w64(x != 0ull) == 0ull) continue;  // word unused by this build (wave-uniform)
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(x, off);
      x = (q == 1) ? (o > x ? o : x) : x + o;
    }
    if ((threadIdx.x & 63) == 0) {
      if (q == 1) atomicMax(&acc[q], x); else atomicAdd(&acc[q], x);
    }
  }
  __syncthreads();
  if (threadIdx.x < NW) {
    const unsigned long long r = acc[threadIdx.x];
    if (r) {
      if (threadIdx.x == 1) atomicMax(&out[1], r); else atomicAdd(&out[threadIdx.x], r);
    }
  }
}

// ---- the three steps both counting sorts below share (a block of CTR_COST_BINS threads, thread t owns scan[t]) ----
// The block's largest key from every thread's largest `m`, as float bits: the top of the cost classes.  smax was set to 1
// before the last barrier.
__device__ __forceinline__ uint32_t block_top(uint32_t m, uint32_t &smax) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0) atomicMax(&smax, m);
  __syncthreads();
  return __float_as_uint((float)smax);
}
// the counter of key c, item i: 64 classes (8 per octave below the maximum) x 16 sub-bins by item index
__device__ __forceinline__ uint32_t cost_bin(uint32_t top, uint32_t c, uint32_t i) {
  const uint32_t fb = __float_as_uint((float)c);       // exponent | mantissa: log-linear in c
  uint32_t cls = fb < top ? (top - fb) >> 20 : 0u;     // 1/8 octave steps below the maximum
  cls = cls > 63u ? 63u : cls;
  return cls * 16u + (i & 15u);
}
// scan[t], the count of bin t once every thread has arrived, becomes the exclusive offset of bin t
__device__ __forceinline__ void scan_bins(uint32_t *scan, uint32_t *wsum) {
  const uint32_t t = threadIdx.x, ln = t & 63u, wv = t >> 6;
  __syncthreads();
  const uint32_t v = scan[t];
  uint32_t x = v;  // inclusive scan inside the wave, then across the 16 waves
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)x, off);
    if (ln >= (uint32_t)off) x += o;
  }
  if (ln == 63u) wsum[wv] = x;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t q = 0; q < wv; q++) base += wsum[q];
  scan[t] = base + x - v;
  __syncthreads();
}

// The same counting sort (see order_block) over groups of GROUP_TILES horizontally adjacent tiles: a group's key is
// the cost of its most expensive tile, its tiles are emitted consecutively.
__device__ void order_block_groups(const uint32_t *__restrict__ cost, uint32_t *__restrict__ order, uint32_t n, uint32_t tiles_x) {
  __shared__ uint32_t scan[CTR_COST_BINS];
  __shared__ uint32_t wsum[CTR_COST_BINS / 64];
  __shared__ uint32_t smax;
  const uint32_t t = threadIdx.x;
  const uint32_t groups_x = (tiles_x + GROUP_TILES - 1) / GROUP_TILES;
  const uint32_t n_groups = (n / tiles_x) * groups_x;  // (single frame: n = tiles_x * tiles_y)
  auto group = [&](uint32_t g, uint32_t &tile0, uint32_t &nt) -> uint32_t {  // -> the group's key
    const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
    tile0 = gy * tiles_x + gx * GROUP_TILES;
    nt = tiles_x - gx * GROUP_TILES < GROUP_TILES ? tiles_x - gx * GROUP_TILES : GROUP_TILES;
    uint32_t c = 0;
    for (uint32_t k = 0; k < nt; k++) c = cost[tile0 + k] > c ? cost[tile0 + k] : c;
    return c;
  };
  scan[t] = 0u;
  if (t == 0) smax = 1u;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t g = t; g < n_groups; g += CTR_COST_BINS) {
    uint32_t tile0, nt;
    const uint32_t c = group(g, tile0, nt);
    m = c > m ? c : m;
  }
  const uint32_t top = block_top(m, smax);
  for (uint32_t g = t; g < n_groups; g += CTR_COST_BINS) {
    uint32_t tile0, nt;
    const uint32_t c = group(g, tile0, nt);
    atomicAdd(&scan[cost_bin(top, c, g)], nt);
  }
  scan_bins(scan, wsum);
  for (uint32_t g = t; g < n_groups; g += CTR_COST_BINS) {
    uint32_t tile0, nt;
    const uint32_t c = group(g, tile0, nt);
    uint32_t at = atomicAdd(&scan[cost_bin(top, c, g)], nt);
    if (CTR_CHEAP_FIRST_PCT && tiles_x % GROUP_TILES == 0) {  // (every group is whole)
      // the cheapest groups first, then the rest from the dearest down: the link to the host has something to carry
      // from the start, while the dear tiles — which complete late whatever the order — are under way
      const uint32_t tail = (uint32_t)((uint64_t)n_groups * CTR_CHEAP_FIRST_PCT / 100u) * GROUP_TILES;  // tiles moved to the front
      at = at >= n - tail ? (n - nt - at) : at + tail;   // (the front in ascending cost)
    }
    for (uint32_t k = 0; k < nt; k++) order[at + k] = tile0 + k;
  }
}

// block of CTR_COST_BINS threads: counting sort of the launch's waves by cost class, expensive first:
// order[slot] = wave.  The sub-bins (cost_bin) only spread the LDS atomics of neighbouring waves, which usually share
// a class.  Any permutation is a correct order; cost only shapes the tail of the next launches.
// tiles_x != 0: keep the GROUP_TILES tiles of a host-delivery group together (sorted by the group's cost), so that
// a group completes — and its pixels leave for the host — soon after its first tile starts.
__device__ void order_block(const uint32_t *__restrict__ cost, uint32_t *__restrict__ order, uint32_t n, uint32_t tiles_x) {
  if (tiles_x) {
    order_block_groups(cost, order, n, tiles_x);
    return;
  }
  __shared__ uint32_t scan[CTR_COST_BINS];
  __shared__ uint32_t wsum[CTR_COST_BINS / 64];
  __shared__ uint32_t smax;
  constexpr uint32_t U = 8;
  const uint32_t t = threadIdx.x;
  scan[t] = 0u;
  if (t == 0) smax = 1u;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += U * CTR_COST_BINS) {
    uint32_t c[U];
#pragma unroll
    for (uint32_t k = 0; k < U; k++) {
      const uint32_t i = b0 + k * CTR_COST_BINS + t;
      c[k] = i < n ? cost[i] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < U; k++) m = c[k] > m ? c[k] : m;
  }
  const uint32_t top = block_top(m, smax);
  for (uint32_t b0 = 0; b0 < n; b0 += U * CTR_COST_BINS) {
    uint32_t c[U];
#pragma unroll
    for (uint32_t k = 0; k < U; k++) {
      const uint32_t i = b0 + k * CTR_COST_BINS + t;
      c[k] = i < n ? cost[i] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < U; k++) {
      const uint32_t i = b0 + k * CTR_COST_BINS + t;
      if (i < n) atomicAdd(&scan[cost_bin(top, c[k], i)], 1u);
    }
  }
  scan_bins(scan, wsum);
  for (uint32_t b0 = 0; b0 < n; b0 += U * CTR_COST_BINS) {
    uint32_t c[U];
#pragma unroll
    for (uint32_t k = 0; k < U; k++) {
      const uint32_t i = b0 + k * CTR_COST_BINS + t;
      c[k] = i < n ? cost[i] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < U; k++) {
      const uint32_t i = b0 + k * CTR_COST_BINS + t;
      if (i < n) order[atomicAdd(&scan[cost_bin(top, c[k], i)], 1u)] = i;
    }
  }
}

// ---- first_order: the dispatch order of a shape nothing is known about yet ----
// Without measured costs the expensive tiles cannot be started first, but a prior helps: what a frame is about sits
// near its centre, walls and sky at its borders.  Tiles are dispatched in blocks of 16x16 tiles, the blocks by their
// (aspect-normalised) distance from the image centre; list-scheduling the measured costs of the shipped scenes puts
// this 6-15 % below image order (border-in: 5-13 % above; DESIGN.md "First launch").  One thread per tile.
__global__ __launch_bounds__(256) void first_order(uint32_t *__restrict__ order, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_frames) {
  const uint32_t tiles_frame = tiles_x * tiles_y;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tiles_frame) return;
  constexpr uint32_t B = 16;
  const uint32_t nbx = (tiles_x + B - 1) / B, nby = (tiles_y + B - 1) / B;
  const uint32_t tx = t % tiles_x, ty = t / tiles_x, bx = tx / B, by = ty / B, me = by * nbx + bx;
  const float aspect = (float)nbx / (float)nby;
  auto key = [&](uint32_t x, uint32_t y) -> float {
    const float dx = ((float)x + 0.5f) - 0.5f * (float)nbx, dy = (((float)y + 0.5f) - 0.5f * (float)nby) * aspect;
    return dx * dx + dy * dy;
  };
  const float km = key(bx, by);
  uint32_t before = 0;  // tiles of the blocks that come first
  for (uint32_t y = 0; y < nby; y++)
    for (uint32_t x = 0; x < nbx; x++) {
      const float k = key(x, y);
      if (k < km || (k == km && y * nbx + x < me)) {
        const uint32_t cw = tiles_x - x * B < B ? tiles_x - x * B : B, ch = tiles_y - y * B < B ? tiles_y - y * B : B;
        before += cw * ch;
      }
    }
  const uint32_t bw = tiles_x - bx * B < B ? tiles_x - bx * B : B;
  const uint32_t slot = before + (ty - by * B) * bw + (tx - bx * B);
  for (uint32_t f = 0; f < n_frames; f++) order[f * tiles_frame + slot] = f * tiles_frame + t;
}

static_assert(CTR_SHARDS == CTR_COST_BINS, "after_render uses one block size for both jobs");
__global__ __launch_bounds__(CTR_SHARDS) void after_render(unsigned long long *__restrict__ shards,
                                                           unsigned long long *__restrict__ counters,
                                                           const uint32_t *__restrict__ cost,
                                                           uint32_t *__restrict__ order, uint32_t n, uint32_t group_tiles_x) {
  if (blockIdx.x == 0) {
    if (shards) fold_block(shards, counters);
  } else {
    if (cost) order_block(cost, order, n, group_tiles_x);
  }
}

}  // namespace

void ctr_launch_first_order(const RenderLaunch &L, hipStream_t stream) {
  const uint32_t nx = tiles_x(L.w), ny = tiles_y(L.rows.n_rows);
  hipLaunchKernelGGL(first_order, dim3((nx * ny + 255) / 256), dim3(256), 0, stream, const_cast<uint32_t *>(L.order), nx, ny,
                     L.n_frames);
}

void ctr_launch_after_render(unsigned long long *shards, unsigned long long *counters, const uint32_t *cost, uint32_t *order,
                             uint32_t n, uint32_t group_tiles_x, hipStream_t stream) {
  hipLaunchKernelGGL(after_render, dim3(cost ? 2 : 1), dim3(CTR_SHARDS), 0, stream, shards, counters, cost, order, n,
                     group_tiles_x);
}

uint64_t ctr_launch_waves(const RenderLaunch &L) { return (uint64_t)tiles_x(L.w) * tiles_y(L.rows.n_rows) * L.n_frames; }
uint64_t ctr_staging_pixels(const RenderLaunch &L) { return ctr_launch_waves(L) * 64u; }
uint64_t ctr_staging_groups(const RenderLaunch &L) {
  const uint64_t nx = tiles_x(L.w), ny = tiles_y(L.rows.n_rows);
  return ((nx + GROUP_TILES - 1) / GROUP_TILES) * ny;
}
uint32_t ctr_group_tile_count(const RenderLaunch &L, uint64_t group) {
  const uint32_t nx = tiles_x(L.w), groups_x = (nx + GROUP_TILES - 1) / GROUP_TILES;
  const uint32_t gx = (uint32_t)(group % groups_x);
  return nx - gx * GROUP_TILES < GROUP_TILES ? nx - gx * GROUP_TILES : GROUP_TILES;
}
uint64_t ctr_staging_index(const RenderLaunch &L, uint32_t x, uint32_t k_row) {
  const uint64_t nx = tiles_x(L.w);
  return ((uint64_t)(k_row / TH) * nx + x / TW) * 64u + (k_row % TH) * TW + x % TW;
}
