// tile_shape.h — the pixel tile of one wave and what follows from it: the one thing the render kernel (render_kernel.hip),
// its launch and the tile scheduler (tile_order.hip) have to agree on.  Host and device; build options CTR_TW, CTR_TH,
// CTR_WAVES_PER_WG.
#ifndef CUTRACE_AMD_TILE_SHAPE_H
#define CUTRACE_AMD_TILE_SHAPE_H

#include <stdint.h>

#ifndef CTR_TW
#define CTR_TW 8
#endif
#ifndef CTR_TH
#define CTR_TH 8
#endif
#ifndef CTR_WAVES_PER_WG
#define CTR_WAVES_PER_WG 1
#endif
constexpr int TW = CTR_TW, TH = CTR_TH;  // pixel tile of one wave (TW*TH == 64)
static_assert(TW * TH == 64, "one wave = one TW x TH tile");
constexpr int WAVES_PER_WG = CTR_WAVES_PER_WG;
constexpr int WG_THREADS = 64 * WAVES_PER_WG;
// tiles of a host-delivery group: 64/TW horizontally adjacent tiles, 64 x TH pixels (render_kernel.hip "Host delivery")
constexpr uint32_t GROUP_TILES = 64 / TW;

// tiles across a frame `w` pixels wide / down the `n_rows` local rows of a launch (DRows::n_rows)
constexpr uint32_t tiles_x(uint32_t w) { return (w + TW - 1) / TW; }
constexpr uint32_t tiles_y(uint32_t n_rows) { return (n_rows + TH - 1) / TH; }

#endif
