// tile_order_policy.h — the tile scheduler's rule (needs no HIP): which launches dispatch by the stored tile order, which start a
// shape centre-out, and which rebuild the order.  No result depends on it (every order renders the same bits), so only
// scripts/tile_order_policy_check.cpp with tests/test_tile_order_policy_cpu.py, and a benchmark, can see a slip here.
// tile_order_host.cpp applies the plan to a launch; the kernels it names are tile_order.hip's.
#ifndef CUTRACE_AMD_TILE_ORDER_POLICY_H
#define CUTRACE_AMD_TILE_ORDER_POLICY_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "cutrace_amd.h"

#ifndef CTR_FIRST_ORDER_MIN_TILES
#define CTR_FIRST_ORDER_MIN_TILES 8192  // smaller launches start in image order: one round of waves, no tail to shape
#endif
#ifndef CTR_ORDER_PERIOD
#define CTR_ORDER_PERIOD 8  // launches between rebuilds of the tile order
#endif

// What a handle remembers between launches (include/cutrace_amd.h "Tile scheduling").
struct OrderState {
  bool valid = false;   // the order buffer holds an order measured on the shape `key`
  uint64_t key[6] = {0, 0, 0, 0, 0, 0};  // the shape: key[0] the number of tiles, the rest frame size, rows, parts, delivery, frames
  uint32_t age = 0;     // launches of the current shape
  uint64_t view = 0;    // camera set + first frame of the previous launch
  size_t cap = 0;       // tiles the cost and order buffers hold
};

struct OrderPlan {
  bool use_order;    // dispatch by the order buffer
  bool order_init;   // ... after filling it centre-out (tile_order.hip first_order)
  bool record_cost;  // the launch writes its tiles' costs; false: no scheduling at all, and the state was not touched
  bool write_next;   // the launch sorts them into the order buffer for the next one
};

// The plan of a launch of shape `key` and view `view`, and the state after it.  heavy: the scene has the triangle count
// that also picks the 6-wave build; variant_bits: the handle's CTR_VAR_*; count: a counting launch.
inline OrderPlan plan_order(OrderState &S, const uint64_t key[6], uint64_t view, bool heavy, uint32_t variant_bits, bool count) {
  OrderPlan P{false, false, false, false};
  const uint64_t n = key[0];
  if ((variant_bits & (CTR_VAR_NO_REORDER | CTR_VAR_STATS)) || count || n == 0 || n > 0x7FFFFFFFull) return P;
  if (n > S.cap) {  // the buffers are regrown: new ones hold no order
    S.valid = false;
    S.cap = (size_t)n;
  }
  const bool same = S.valid && memcmp(key, S.key, sizeof(S.key)) == 0;
  // (a shape's first launch runs in image order: an a-priori estimate — tiles whose primary rays meet the box
  //  of a mesh / sphere, computed and sorted by a pre-pass — was built and measured in round 2: the expensive
  //  tiles of these scenes are speckle along shadow edges and reflections, not the tiles that look at an
  //  object, and the pre-pass cost more than it won; DESIGN.md "First launch")
  if (same) P.use_order = true;
  else {
    S.age = 0;
    // a shape nothing is known about: centre-out instead of image order (tile_order.hip first_order) — for
    // launches large enough to have a tail and scenes heavy enough for the ~8 us of the order kernel to pay:
    // bunny -5.5 %, 64k bunny -2 %, C4 -2 %, but mirror.json (924 triangles, 0.2 ms) +4 %
    // (profiles/r02/first_launch_centre_out.txt)
    if (n >= CTR_FIRST_ORDER_MIN_TILES && heavy && !(variant_bits & CTR_VAR_IMAGE_ORDER_FIRST)) P.use_order = P.order_init = true;
  }
  memcpy(S.key, key, sizeof(S.key));
  S.valid = true;  // after this launch the order buffer holds an order measured on this shape
  P.record_cost = true;
  // The order is rebuilt after the first two launches of a shape (the second one measured under the
  // new order); after that every launch while the view keeps changing (a camera path: 90-frame
  // orbit 1.46 ms/frame rebuilt every frame vs 1.59 every 8th, 1.77 without scheduling), and only
  // every CTR_ORDER_PERIOD-th launch while the same view is rendered again and again.
  const bool same_view = same && view == S.view;
  S.view = view;
  P.write_next = S.age < 2 || !same_view || S.age % CTR_ORDER_PERIOD == 0;
  S.age++;
  return P;
}

#endif
