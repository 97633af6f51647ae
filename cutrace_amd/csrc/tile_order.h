// tile_order.h — the tile scheduler (tile_order.hip): the launch's tile and staging geometry for the host, and the two small
// kernels that run around the render kernel on its stream.  Host declarations; nothing here is part of the C-ABI.
#ifndef CUTRACE_AMD_TILE_ORDER_H
#define CUTRACE_AMD_TILE_ORDER_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "cutrace_amd.h"
#include "scene_device.h"

#pragma GCC visibility push(hidden)
// number of waves (tiles x frames) the launch will dispatch
uint64_t ctr_launch_waves(const RenderLaunch &L);
// "Host delivery" (render_kernel.hip): pixels per staging buffer, groups of tiles, and where a pixel lies in the staging area
uint64_t ctr_staging_pixels(const RenderLaunch &L);
uint64_t ctr_staging_groups(const RenderLaunch &L);
uint32_t ctr_group_tile_count(const RenderLaunch &L, uint64_t group);          // tiles group `group` counts when it is complete
uint64_t ctr_staging_index(const RenderLaunch &L, uint32_t x, uint32_t k_row); // staging pixel of compact pixel (x, k_row)

// before the render: fills L.order with the centre-out order of the launch's tiles, every frame alike (first_order)
void ctr_launch_first_order(const RenderLaunch &L, hipStream_t stream);
// after the render (after_render): one block adds the counter shards into `counters` and clears them (null shards: nothing
// to fold); with `cost`, a second block sorts the launch's `n` waves by it into `order` — group_tiles_x != 0: the tiles
// of a host-delivery group stay together, the frame being group_tiles_x tiles wide
void ctr_launch_after_render(unsigned long long *shards, unsigned long long *counters, const uint32_t *cost, uint32_t *order,
                             uint32_t n, uint32_t group_tiles_x, hipStream_t stream);

// tile_order_host.cpp: attaches the handle's tile-order buffers to a launch by the rule of tile_order_policy.h: the launch uses the
// stored order when it has the shape the order was measured on, records its costs and sorts them for the next one.  heavy: the
// scene has the triangle count that also picks the 6-wave build.
int attach_order(ctr_scene *s, RenderLaunch &L, bool heavy, bool count);
#pragma GCC visibility pop

#endif
