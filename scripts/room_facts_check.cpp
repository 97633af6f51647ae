// room_facts_check.cpp — the lemma behind the room facts (cutrace_amd/csrc/scene_flatten.cpp room_facts; DESIGN.md "Shadow casts
// from inside a plane room"), looked for counter-examples on the CPU, in float, before any GPU time is spent on it.  No HIP.
//
//   room_facts_check [samples] [--k-div X] [--delta-mul X] [--seed N]     the search; prints one "checked ..." line
//   room_facts_check scene <scene.bin>                                    the facts of a scene file, one "facts ..." line
//
// The search draws rooms of axis-aligned planes (six, five with one side open, one to three single planes; sizes 1e-3 .. 1e3,
// offsets up to 1e4, normals of any length), point lights (inside, next to a wall, exactly at the margin by bisection on the
// facts themselves, outside a wall) and suns, asks room_facts for the six words, and then draws origins where the lemma can
// break: numerators within +-2 delta of a wall, on the faces of the origin box, opposite the wall a light hugs, level with a
// light (denominator near zero), and plain ones.  For every origin that passes the lane predicate exactly as the kernel
// evaluates it, and every light whose bit is set, the shadow ray and plane::intersect are restated in float as the reference
// computes them (shading.hpp:32,80; default_schema.hpp:189-201,305-308; vector.hpp: dot left to right, normalized() = a * (1 / norm))
// and the planes that occlude — isfinite(t0) && t0 > min_t && t0 < light_dist — are counted.  The count must be 0.
// --k-div / --delta-mul mutate the facts (RoomTuning): the search has to find violations then, or it proves nothing.
// scene.bin: the format of scripts/flatten_check.cpp.  CUTRACE_NO_WALL_SKIP is honoured as the library honours it.
// Build with -ffp-contract=off (every float operation rounded once), e.g.
//   g++ -std=c++17 -O2 -ffp-contract=off -Icutrace_amd/csrc -Iinclude scripts/room_facts_check.cpp cutrace_amd/csrc/scene_flatten.cpp
//       cutrace_amd/csrc/guard.cpp cutrace_amd/csrc/bvh.cpp -pthread
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scene_flatten.h"

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double u() { return (double)(next() >> 11) * 0x1p-53; }            // [0, 1)
  double u(double a, double b) { return a + (b - a) * u(); }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct V { float x, y, z; float &operator[](int a) { return a == 0 ? x : a == 1 ? y : z; } float operator[](int a) const { return a == 0 ? x : a == 1 ? y : z; } };
float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }   // vector.hpp: left to right
float norm(V a) { return sqrtf(dot(a, a)); }
V normalized(V a) { const float inv = 1.0f / norm(a); return {a.x * inv, a.y * inv, a.z * inv}; }
float ulps(float x, int k) { for (int i = 0; i < abs(k); i++) x = nextafterf(x, k > 0 ? INFINITY : -INFINITY); return x; }

struct Plane { V p, n; int axis; };
struct Room {
  DSceneHead H{};
  std::vector<Plane> planes;   // the filled slots, full records (the components the head does not hold: any point, zero normal)
  std::vector<DLight> lights;
  double lo[3], hi[3], scale;
};

void make_room(Rng &R, Room &rm) {
  rm = Room();
  const double scale = pow(10.0, R.u(-3, 3));
  rm.scale = scale;
  double off[3];
  for (int a = 0; a < 3; a++) {
    off[a] = R.below(3) == 0 ? 0.0 : R.u(-1, 1) * pow(10.0, R.u(0, 4));
    const double h = scale * R.u(0.5, 3);
    rm.lo[a] = (float)(off[a] - h); rm.hi[a] = (float)(off[a] + h);
  }
  // which slots exist: 6, 5 (one open side), or 1..3 single planes
  bool filled[6];
  const uint32_t kind = R.below(4);
  for (int k = 0; k < 6; k++) filled[k] = kind <= 1;
  if (kind == 1) filled[R.below(6)] = false;
  if (kind >= 2) { const uint32_t n = 1 + R.below(3); for (uint32_t i = 0; i < n; i++) filled[R.below(6)] = true; }
  rm.H.n_axis_recs = 3u;
  for (int k = 0; k < 6; k++) {
    const int a = k / 2, side = k & 1;  // side 0: the wall at lo, normal +; side 1: the wall at hi, normal -
    rm.H.ax_index[k] = filled[k] ? (uint32_t)k : CTR_PLANE_PAD;
    const float nlen = R.below(3) == 0 ? (float)pow(10.0, R.u(-2, 2)) : 1.0f;
    const float p = (float)(side ? rm.hi[a] : rm.lo[a]), n = side ? -nlen : nlen;
    rm.H.ax[2 * a][side] = p; rm.H.ax[2 * a + 1][side] = n;
    if (filled[k]) {
      Plane P{};
      for (int q = 0; q < 3; q++) { P.p[q] = (float)R.u(rm.lo[q], rm.hi[q]); P.n[q] = 0.0f; }
      P.p[a] = p; P.n[a] = n; P.axis = a;
      rm.planes.push_back(P);
    }
  }
  // an empty slot copies its neighbour, as plane_records leaves it (never tested; the kernel's maximum runs over it)
  for (int a = 0; a < 3; a++)
    for (int s = 0; s < 2; s++)
      if (!filled[2 * a + s] && filled[2 * a + 1 - s]) { rm.H.ax[2 * a][s] = rm.H.ax[2 * a][1 - s]; rm.H.ax[2 * a + 1][s] = rm.H.ax[2 * a + 1][1 - s]; }
      else if (!filled[2 * a] && !filled[2 * a + 1]) { rm.H.ax[2 * a][s] = 0.0f; rm.H.ax[2 * a + 1][s] = 1.0f; }
  const uint32_t n_light = 1 + R.below(4);
  for (uint32_t i = 0; i < n_light; i++) {
    DLight L{};
    L.type = R.below(8) == 0 ? CTR_LIGHT_SUN : CTR_LIGHT_POINT;
    float v[3];
    for (int a = 0; a < 3; a++) v[a] = (float)R.u(rm.lo[a], rm.hi[a]);
    const uint32_t how = R.below(4);
    if (how >= 1) {  // next to a wall: 1e-7 .. 0.3 of the scale inside it (how == 3: outside)
      const int k = (int)R.below(6), a = k / 2;
      const double d = scale * pow(10.0, R.u(-7, -0.5)) * (how == 3 ? -1.0 : 1.0);
      v[a] = (float)((k & 1) ? rm.hi[a] - d : rm.lo[a] + d);
    }
    L.vx = v[0]; L.vy = v[1]; L.vz = v[2];
    rm.lights.push_back(L);
  }
}

// light `i` moved along `a` to the smallest distance from the wall of slot k at which the facts still give it its bit
void to_the_margin(Room &rm, const RoomTuning &tune, uint32_t i, int k) {
  const int a = k / 2;
  const bool hi_side = k & 1;
  float *v = a == 0 ? &rm.lights[i].vx : a == 1 ? &rm.lights[i].vy : &rm.lights[i].vz;
  const float wall = (float)(hi_side ? rm.hi[a] : rm.lo[a]);
  double near = 0.0, far = 0.4 * (rm.hi[a] - rm.lo[a]);
  auto has_bit = [&](double d) { *v = (float)(hi_side ? wall - d : wall + d); DSceneHead H = rm.H; room_facts(H, rm.lights.data(), rm.lights.size(), tune); return ((H.room_lights >> i) & 1u) != 0u; };
  if (!has_bit(far)) return;
  for (int it = 0; it < 60; it++) { const double mid = 0.5 * (near + far); (has_bit(mid) ? far : near) = mid; }
  has_bit(far);
}

struct Tally { uint64_t origins = 0, safe_origins = 0, pairs = 0, plane_tests = 0, violations = 0, cases[5] = {0, 0, 0, 0, 0}; };

// W(o), as the kernel evaluates it: the six numerators of the head's slots, the tolerance, the box
bool lane_predicate(const DSceneHead &H, V o) {
  float m = -INFINITY;
  for (int a = 0; a < 3; a++)
    for (int s = 0; s < 2; s++) m = fmaxf(m, (H.ax[2 * a][s] - o[a]) * H.ax[2 * a + 1][s]);
  const bool in_box = fabsf(o.x - H.room_c[0]) <= H.room_r && fabsf(o.y - H.room_c[1]) <= H.room_r && fabsf(o.z - H.room_c[2]) <= H.room_r;
  return in_box && m <= H.room_delta;
}

void check_origin(const Room &rm, const DSceneHead &H, V o, Tally &T, bool verbose) {
  T.origins++;
  if (!lane_predicate(H, o)) return;
  T.safe_origins++;
  const float min_t = (float)(0.0 + 1e-3);
  for (size_t i = 0; i < rm.lights.size(); i++) {
    if (!((H.room_lights >> i) & 1u)) continue;
    T.pairs++;
    const V L{rm.lights[i].vx, rm.lights[i].vy, rm.lights[i].vz};
    const V diff{L.x - o.x, L.y - o.y, L.z - o.z};
    const V dir0 = normalized(diff), d = normalized(dir0);
    const float light_dist = norm(diff) * norm(dir0);
    for (const Plane &P : rm.planes) {
      const V po{P.p.x - o.x, P.p.y - o.y, P.p.z - o.z};
      const float num = dot(po, P.n), den = dot(d, P.n), t0 = num / den;
      T.plane_tests++;
      T.cases[!(den == den) || den == 0.0f ? 4 : num <= 0.0f ? (den > 0.0f ? 0 : 1) : (den > 0.0f ? 2 : 3)]++;
      if (std::isfinite(t0) && t0 > min_t && t0 < light_dist) {
        if (verbose && T.violations < 5)
          fprintf(stderr, "violation: axis %d p %.9g n %.9g  o %.9g  L %.9g  num %.9g den %.9g t0 %.9g light_dist %.9g delta %.9g scale %.3g\n", P.axis,
                  P.p[P.axis], P.n[P.axis], o[P.axis], L[P.axis], num, den, t0, light_dist, H.room_delta, rm.scale);
        T.violations++;
      }
    }
  }
}

V draw_origin(Rng &R, const Room &rm, const DSceneHead &H) {
  V o;
  for (int a = 0; a < 3; a++) o[a] = (float)R.u(rm.lo[a], rm.hi[a]);
  const uint32_t how = R.below(8);
  const int k = (int)R.below(6), a = k / 2, s = k & 1;
  const float p = H.ax[2 * a][s], n = H.ax[2 * a + 1][s];
  switch (how) {
    case 0: break;                                                                            // anywhere in the room
    case 1: o[a] = (float)((double)p - R.u(-2, 2) * (double)H.room_delta / (double)n); break;   // numerator within +-2 delta
    case 2: o[a] = ulps(p, (int)R.below(9) - 4); break;                                       // on the wall, a few ulp either side
    case 3: o[a] = ulps(H.room_c[a] + (s ? H.room_r : -H.room_r), (int)R.below(5) - 2); break;  // a face of the origin box
    case 4: {                                                                                 // level with a light: den near 0
      const DLight &L = rm.lights[R.below((uint32_t)rm.lights.size())];
      o[a] = ulps(a == 0 ? L.vx : a == 1 ? L.vy : L.vz, (int)R.below(7) - 3);
      break;
    }
    case 5: o[a] = ulps(H.ax[2 * a][1 - s], s ? -(int)R.below(4) : (int)R.below(4)); break;   // on the opposite wall: the largest s_o
    case 6: for (int q = 0; q < 3; q++) o[q] = (float)(H.room_c[q] + R.u(-1, 1) * H.room_r); break;  // anywhere in the box
    default: {                                                                                // a corner region, far from everything
      for (int q = 0; q < 3; q++) o[q] = ulps((float)(R.below(2) ? rm.hi[q] : rm.lo[q]), (int)R.below(5) - 2);
      break;
    }
  }
  if (R.below(4) == 0) {  // and a second coordinate on a wall as well: a hit point near an edge
    const int k2 = (int)R.below(6);
    o[k2 / 2] = ulps(H.ax[2 * (k2 / 2)][k2 & 1], (int)R.below(5) - 2);
  }
  return o;
}

template <class T> std::vector<T> read_array(FILE *f, uint64_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "room_facts_check: short scene file\n"); exit(3); }
  return v;
}

int scene_mode(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); return 3; }
  const std::vector<uint64_t> n = read_array<uint64_t>(f, 5);
  const auto objects = read_array<ctr_object>(f, n[0]);
  const auto triangles = read_array<ctr_triangle>(f, n[1]);
  const auto lights = read_array<ctr_light>(f, n[2]);
  const auto materials = read_array<ctr_material>(f, n[3]);
  ctr_scene_desc d{objects.data(), n[0], triangles.data(), n[1], lights.data(), n[2], materials.data(), n[3], read_array<ctr_camera>(f, 1)[0]};
  fclose(f);
  std::string err;
  FlatScene F;
  if (validate_desc(d, err) || flatten_scene(d, F, err)) { printf("invalid: %s\n", err.c_str()); return 2; }
  DSceneHead H;
  fill_scene_head(F, F.tlas_root, H);
  fill_room_facts(F, H, env_switch("CUTRACE_NO_WALL_SKIP"));
  // does the box hold the triple's plane points and the point lights?
  bool holds = true;
  for (int k = 0; k < 6; k++)
    if (H.ax_index[k] != CTR_PLANE_PAD) holds = holds && fabsf(H.ax[2 * (k / 2)][k & 1] - H.room_c[k / 2]) <= H.room_r;
  for (const DLight &L : F.lights)
    if (L.type == CTR_LIGHT_POINT) holds = holds && fabsf(L.vx - H.room_c[0]) <= H.room_r && fabsf(L.vy - H.room_c[1]) <= H.room_r && fabsf(L.vz - H.room_c[2]) <= H.room_r;
  printf("facts c %.9g %.9g %.9g r %.9g delta %.9g lights 0x%x box_holds %d n_axis_recs %u plane_recs %zu all_opaque %d\n", H.room_c[0], H.room_c[1],
         H.room_c[2], H.room_r, H.room_delta, H.room_lights, holds ? 1 : 0, F.n_axis_recs, F.planes.size(), F.all_opaque ? 1 : 0);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "scene")) return scene_mode(argv[2]);
  uint64_t samples = 20000000ull, seed = 1;
  RoomTuning tune;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--k-div") && i + 1 < argc) tune.k /= atof(argv[++i]);
    else if (!strcmp(argv[i], "--delta-mul") && i + 1 < argc) tune.delta_scale *= atof(argv[++i]);
    else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
    else samples = strtoull(argv[i], nullptr, 10);
  }
  Rng R{seed * 0x2545F4914F6CDD1Dull + 12345};
  Tally T;
  uint64_t rooms = 0, rooms_with_facts = 0;
  const uint32_t per_room = 64;
  while (T.origins < samples) {
    Room rm;
    make_room(R, rm);
    if (R.below(2) == 0) {  // a light exactly at the margin of a wall (of a filled slot, if it finds one)
      const uint32_t i = R.below((uint32_t)rm.lights.size());
      int k = (int)R.below(6);
      for (int t = 0; t < 6 && rm.H.ax_index[k] == CTR_PLANE_PAD; t++) k = (k + 1) % 6;
      if (rm.lights[i].type == CTR_LIGHT_POINT && rm.H.ax_index[k] != CTR_PLANE_PAD) to_the_margin(rm, tune, i, k);
    }
    DSceneHead H = rm.H;
    room_facts(H, rm.lights.data(), rm.lights.size(), tune);
    rooms++;
    if (H.room_lights == 0u) {
      // nothing may be claimed: every word zero
      if (H.room_r != 0.0f || H.room_delta != 0.0f || H.room_c[0] != 0.0f || H.room_c[1] != 0.0f || H.room_c[2] != 0.0f) { printf("FAIL: no light qualifies but the words are not zero\n"); return 1; }
      T.origins += 4;  // (counts towards the budget, so that the loop ends whatever the share of such rooms)
      continue;
    }
    rooms_with_facts++;
    for (uint32_t j = 0; j < per_room; j++) check_origin(rm, H, draw_origin(R, rm, H), T, true);
  }
  printf("checked rooms %llu with_facts %llu origins %llu safe_origins %llu safe_pairs %llu plane_tests %llu cases a %llu b %llu c %llu c' %llu d %llu violations %llu (k %.6g delta_scale %.6g)\n",
         (unsigned long long)rooms, (unsigned long long)rooms_with_facts, (unsigned long long)T.origins, (unsigned long long)T.safe_origins,
         (unsigned long long)T.pairs, (unsigned long long)T.plane_tests, (unsigned long long)T.cases[0], (unsigned long long)T.cases[1],
         (unsigned long long)T.cases[2], (unsigned long long)T.cases[3], (unsigned long long)T.cases[4], (unsigned long long)T.violations, tune.k,
         tune.delta_scale);
  return 0;
}
