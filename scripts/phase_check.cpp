// phase_check.cpp — the invariant behind the phased builds (cutrace_amd/csrc/render_kernel.hip "Phased builds", render_trip.h;
// DESIGN.md "Phased opaque builds"), looked for counter-examples on the CPU before any GPU time is spent on it.  No HIP.
//
//   phase_check [waves] [--seed N] [--transparent]
//
// prints one "checked ..." line; exit status 0 when the result is the expected one (no violation — or, under the mutation,
// at least one).  A wave is 64 lanes of the kernel's state machine, modelled abstractly: per lane the mode (radiance, shadow,
// done), the stack depth, the light index `li` and the dark bit; per trip and active lane one draw each for "the ray hit
// something", "the hit's material has reflect >= 1e-6", "an occluder was met" and "this light is dark for the hit".  The
// transitions are the continuation's of an opaque any-hit build:
//   radiance trip: miss -> unwind (every frame waits for its reflection child only, so the lane unwinds to depth 0: done);
//                  hit  -> li = 0; with a light left a shadow cast towards it, else the bounce
//   shadow trip:   the loop of shadow_intensity ends with its first trip (done_shadow); a dark lane sits the trip out but
//                  takes it; li++; with a light left the next shadow cast, else the bounce
//   bounce:        depth < bounces and the material reflects -> depth + 1, a radiance cast; else unwind: done
// Draws: 0 ... 33 lights, bounces 0 ... 15, hit / reflect / occluder / dark probabilities per wave from {0, 0.1, 0.5, 0.9, 1},
// lanes inactive from the start (outside the image, or a masked ray) with probability 0, 0.3 or 0.9 per wave.
// Claim, asserted in every trip: all active lanes share the kind of the cast and, in a shadow trip, `li`; and the scalar rule
//   phase = 0 at the start;  after a trip  phase = (phase == n_light) ? 0 : phase + 1
// predicts both: phase == 0 iff the trip is a radiance trip, else li == phase - 1.  `violations` counts the trips where not.
// The mutation weakens the premise; the search has to find violations under it, or it proves nothing:
//   --transparent   a material transmits, as in the builds that are not any-hit: an occluded lane whose accumulated intensity is
//                   below 1 casts the same shadow ray again (a second trip for the same light), and the lanes drift apart
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double u() { return (double)(next() >> 11) * 0x1p-53; }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
  bool chance(double p) { return u() < p; }
};

enum Mode { RADIANCE, SHADOW, DONE };
struct Lane {
  Mode mode;
  int depth;
  uint32_t li;
  bool dark;
  float intensity;  // --transparent: shadow_intensity's accumulator
};

const double PROB[5] = {0.0, 0.1, 0.5, 0.9, 1.0};

}  // namespace

int main(int argc, char **argv) {
  uint64_t waves = 200000, seed = 1;
  bool transparent = false;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--transparent")) transparent = true;
    else waves = strtoull(argv[i], nullptr, 10);
  }
  Rng R{seed * 0x2545F4914F6CDD1Dull + 12345};
  uint64_t trips = 0, radiance_trips = 0, shadow_trips = 0, violations = 0, lanes_cast = 0, longest = 0;
  for (uint64_t wv = 0; wv < waves; wv++) {
    const uint32_t n_light = wv % 7 == 0 ? 33u : R.below(34);
    const int bounces = (int)R.below(16);
    const double p_hit = PROB[R.below(5)], p_refl = PROB[R.below(5)], p_occ = PROB[R.below(5)], p_dark = PROB[R.below(5)];
    const double p_off = R.below(3) == 0 ? 0.0 : (R.below(2) ? 0.3 : 0.9);
    Lane L[64];
    for (auto &l : L) l = {R.chance(p_off) ? DONE : RADIANCE, 0, 0u, false, 0.f};
    uint32_t phase = 0;
    uint64_t t = 0;
    for (;; t++) {
      // ---- the trip head: who is active, and what for ----
      int n_active = 0, n_rad = 0, n_shadow = 0;
      bool li_same = true;
      uint32_t li0 = 0;
      for (const auto &l : L) {
        if (l.mode == DONE) continue;
        n_active++;
        if (l.mode == RADIANCE) { n_rad++; continue; }
        if (n_shadow == 0) li0 = l.li;                   // the first shadow lane
        else if (l.li != li0) li_same = false;
        n_shadow++;
      }
      if (n_active == 0) break;
      trips++;
      lanes_cast += (uint64_t)n_active;
      const bool mixed = n_rad != 0 && n_rad != n_active;
      const bool is_rad = n_rad == n_active;
      bool ok = !mixed && (is_rad || li_same);
      ok = ok && (is_rad ? phase == 0u : (phase != 0u && li0 == phase - 1u));
      if (!ok) violations++;
      (is_rad ? radiance_trips : shadow_trips)++;
      // ---- the continuation, lane by lane ----
      for (auto &l : L) {
        if (l.mode == DONE) continue;
        bool to_light = false;
        if (l.mode == RADIANCE) {
          if (!R.chance(p_hit)) { l.mode = DONE; continue; }   // miss: unwinds to depth 0 (reflection frames only)
          l.li = 0;
          to_light = true;
        } else {
          const bool occluded = !l.dark && R.chance(p_occ);
          bool done_shadow = true;
          if (transparent && occluded) {
            l.intensity += 0.5f;                               // 1 - transparency of the occluder
            if (l.intensity < 1.0f) done_shadow = false;       // cast again, the same ray
          }
          if (done_shadow) { l.li++; to_light = true; }
        }
        if (!to_light) continue;
        if (l.li < n_light) {
          l.mode = SHADOW;
          l.dark = R.chance(p_dark);
          l.intensity = 0.f;
        } else if (l.depth < bounces && R.chance(p_refl)) {
          l.depth++;
          l.mode = RADIANCE;
          l.dark = false;
        } else {
          l.mode = DONE;
        }
      }
      phase = phase == n_light ? 0u : phase + 1u;
      if (t > 100000) { printf("a wave that does not end\n"); return 2; }
    }
    if (t > longest) longest = t;
  }
  printf("checked %llu waves, %llu trips (%llu radiance, %llu shadow), %llu lane casts, longest wave %llu trips, mutation %s: violations %llu\n",
         (unsigned long long)waves, (unsigned long long)trips, (unsigned long long)radiance_trips, (unsigned long long)shadow_trips,
         (unsigned long long)lanes_cast, (unsigned long long)longest, transparent ? "transparent" : "none", (unsigned long long)violations);
  return (transparent ? violations != 0 : violations == 0) ? 0 : 1;
}
