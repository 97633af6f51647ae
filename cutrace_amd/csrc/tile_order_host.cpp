// tile_order_host.cpp — the host half of the tile scheduler: the handle's order state (tile_order_policy.h OrderState) and its
// two buffers applied to a launch, the costs of the last launch for the caller, and the test hook that spoils an order.
#include "ctr_internal.h"
#include "tile_order.h"

int attach_order(ctr_scene *s, RenderLaunch &L, bool heavy, bool count) {
  L.order = L.order_next = nullptr;
  L.cost = nullptr;
  const uint64_t n = ctr_launch_waves(L);
  const uint64_t key[6] = {n, ((uint64_t)L.w << 32) | L.h, ((uint64_t)L.rows.row_begin << 32) | L.rows.row_end,
                           ((uint64_t)L.rows.block_rows << 32) | L.rows.n_parts,
                           ((uint64_t)L.rows.part << 32) | L.rows.part_stride,
                           ((uint64_t)(L.group_done ? 1u : 0u) << 32) | L.n_frames};  // (host delivery orders tiles by group)
  const uint64_t view = ((uint64_t)s->cams_epoch << 32) | L.first_frame;
  const OrderPlan plan = plan_order(s->order, key, view, heavy, s->user_variant, count);
  if (!plan.record_cost) return CTR_OK;
  if (int st = reserve_both(s->d_cost, s->d_order, s->order.cap)) {
    s->order = OrderState{};  // no buffers, no order: the next launch starts over
    return st;
  }
  uint32_t *const order = s->d_order.as<uint32_t>();
  if (plan.use_order) L.order = order;
  L.order_init = plan.order_init ? 1 : 0;
  L.cost = s->d_cost.as<uint32_t>();
  if (plan.write_next) L.order_next = order;
  if (s->poison_next_order) {
    // test hook: this launch gets an order whose second half names no tile — those waves leave at once, their tiles
    // are never rendered, and (host delivery) their groups never complete
    s->poison_next_order = false;
    std::vector<uint32_t> o(n);
    for (uint64_t k = 0; k < n; k++) o[k] = k < n / 2 ? (uint32_t)k : 0xFFFFFFFFu;
    HIP_TRY(hipMemcpy(order, o.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    L.order = order;
    L.order_init = 0;
    L.order_next = nullptr;
    s->order.valid = false;  // the next launch starts over
  }
  return CTR_OK;
}

extern "C" {

int ctr_debug_poison_next_order(ctr_scene *s) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  std::lock_guard<std::mutex> lk(s->mtx);
  s->poison_next_order = true;
  return CTR_OK;
}

int ctr_tile_costs(ctr_scene *s, uint32_t *out, uint64_t capacity, uint64_t *n_tiles) {
  if (!s) return fail(CTR_E_INVALID, "null scene");
  std::lock_guard<std::mutex> lk(s->mtx);
  const uint64_t n = s->order.valid ? s->order.key[0] : 0;
  if (n_tiles) *n_tiles = n;
  if (out && n) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, s->d_cost.p, sizeof(uint32_t) * (n < capacity ? n : capacity), hipMemcpyDeviceToHost));
  }
  return CTR_OK;
}

}  // extern "C"
