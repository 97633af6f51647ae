// tile_order_policy_check.cpp — feeds plan_order (cutrace_amd/csrc/tile_order_policy.h) scripted sequences of launches for
// tests/test_tile_order_policy_cpu.py: one line per launch,
//   "seq k0 k1 k2 k3 k4 k5 view heavy variant count cap_lost | use_order order_init record_cost write_next age"
// the six key words (k0 = tiles), the launch's other inputs, whether the buffers were lost before it (capacity 0, as a failed
// regrow leaves it), then the plan and the age after the launch.  Host only: g++, no HIP.
#include <stdio.h>

#include <initializer_list>

#include "tile_order_policy.h"

namespace {

struct Shape { uint64_t key[6]; };
const Shape A{{1000, 1, 2, 3, 4, 5}}, A_ROWS{{1000, 1, 9, 3, 4, 5}}, B{{500, 1, 2, 3, 4, 5}}, BIG{{5000, 1, 2, 3, 4, 5}};

struct Launch {
  Shape shape;
  uint64_t view = 7;
  bool heavy = false;
  uint32_t variant = 0;
  bool count = false;
  bool cap_lost = false;
};

void run(const char *seq, OrderState &S, const Launch &l) {
  if (l.cap_lost) S.cap = 0;
  const OrderPlan p = plan_order(S, l.shape.key, l.view, l.heavy, l.variant, l.count);
  const uint64_t *k = l.shape.key;
  printf("%s %llu %llu %llu %llu %llu %llu %llu %d %u %d %d | %d %d %d %d %u\n", seq, (unsigned long long)k[0], (unsigned long long)k[1],
         (unsigned long long)k[2], (unsigned long long)k[3], (unsigned long long)k[4], (unsigned long long)k[5],
         (unsigned long long)l.view, (int)l.heavy, l.variant, (int)l.count, (int)l.cap_lost, (int)p.use_order, (int)p.order_init,
         (int)p.record_cost, (int)p.write_next, S.age);
}

Shape tiles(uint64_t n) { return Shape{{n, 1, 2, 3, 4, 5}}; }

}  // namespace

int main() {
  {  // (a) one shape, one view
    OrderState S;
    for (int i = 0; i < 20; i++) run("a", S, {A});
  }
  {  // (b) the view changes every launch
    OrderState S;
    for (int i = 0; i < 20; i++) run("b", S, {A, (uint64_t)i});
  }
  {  // (c) shape A, a smaller one, A again; then a shape that differs in a later key word only
    OrderState S;
    for (const Shape &s : {A, B, A, A_ROWS})
      for (int i = 0; i < 3; i++) run("c", S, {s});
  }
  {  // (d) a shape beyond the capacity; the same shape after the buffers were lost
    OrderState S;
    for (int i = 0; i < 3; i++) run("d", S, {A});
    for (int i = 0; i < 3; i++) run("d", S, {BIG});
    Launch lost{BIG};
    lost.cap_lost = true;
    run("d", S, lost);
    for (int i = 0; i < 2; i++) run("d", S, {BIG});
  }
  // (e) the centre-out start
  for (uint64_t n : {(uint64_t)CTR_FIRST_ORDER_MIN_TILES - 1, (uint64_t)CTR_FIRST_ORDER_MIN_TILES})
    for (bool heavy : {false, true}) {
      OrderState S;
      for (int i = 0; i < 2; i++) run("e", S, {tiles(n), 7, heavy});
    }
  {
    OrderState S;
    for (int i = 0; i < 2; i++) run("e", S, {tiles(CTR_FIRST_ORDER_MIN_TILES), 7, true, CTR_VAR_IMAGE_ORDER_FIRST});
  }
  {  // (f) launches that are not scheduled, in the middle of (a)
    OrderState S;
    for (int i = 0; i < 20; i++) {
      run("f", S, {A});
      if (i == 4) {
        run("f", S, {A, 7, false, CTR_VAR_NO_REORDER});
        run("f", S, {B, 8, true, CTR_VAR_STATS});
        run("f", S, {BIG, 9, false, 0, true});
        run("f", S, {tiles(0), 9});
        run("f", S, {tiles(0x80000000ull), 9, true});
      }
    }
  }
  return 0;
}
