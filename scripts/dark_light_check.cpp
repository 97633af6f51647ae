// dark_light_check.cpp — the lemma behind the dark-light skip (cutrace_amd/csrc/render_kernel.hip "dark lights",
// cutrace_amd/csrc/scene_flatten.cpp shade_facts; DESIGN.md "Dark lights"), looked for counter-examples on the CPU, in float,
// before any GPU time is spent on it.  No HIP.
//
//   dark_light_check [cases] [--seed N] [--no-neg-zero-guard] [--denormal-is-zero] [--no-bound]
//
// prints one "checked ..." line.  Every case is one (hit, light) pair of phong (shading.hpp:86-94) restated in float, each
// operation rounded once: fd = max(0, nn.nd), h = (-in_dn + nd).normalized(), fs = pow(max(0, nn.h), phong_exp) — as the f64 pow
// rounded once, or as exp2f(e * log2f(x)) with e == 0 -> 1, the two forms the kernels have —, ld = diffuse * colour,
// ls = (diffuse * specular) * colour, term = (ld * fd + ls * fs) * (1 - shadow_fac) with shadow_fac = 0, final = final + term.
// The predicate D is the kernel's:
//   the scene facts hold (shade_facts of the case's material and light: all finite, all within CTR_SHADE_BOUND),
//   fd is +0 or -0 as bits, fs is +0 or -0 as bits (a denormal is not zero), and no channel of `final` is -0 as bits.
// Claim: D  =>  final + term == final, bit for bit in every channel (so whether the shadow cast finds an occluder — the term is
// then not added — or not cannot be seen).  `violations` counts the cases with D where it is not; it must be 0.
// The draws put the weight where the claim can break: signed zeros in every input, negative colours such as (0.5, -0.7, 0.2),
// negative ambient with a zero material colour (final = -0), exponents 0, 0.5, 1, 2, 200, 1000 and 1e5, nn.nd and nn.h within a
// few ulp of 0 on both sides, specular factors that land in the denormals, infinite and NaN colours, and finite colours whose
// product overflows.
// The second claim, counted in `finite_mismatch` (must be 0): bit 0 of shade_facts is clear exactly when some material colour,
// `specular` or light colour of the case is not finite — whatever phong_exp, reflexivity, transparency or the light's position are.
// The mutations weaken D; the search has to find violations under each of them, or it proves nothing:
//   --no-neg-zero-guard   the guard on `final` is dropped        ((-0) + (+0) = +0)
//   --denormal-is-zero    a denormal fs counts as zero           (x + denormal * ls != x)
//   --no-bound            finite colours are enough              (0 * (1e30 * 1e30) = NaN)
// Build with -ffp-contract=off (every float operation rounded once), e.g.
//   g++ -std=c++17 -O2 -ffp-contract=off -Icutrace_amd/csrc -Iinclude scripts/dark_light_check.cpp cutrace_amd/csrc/scene_flatten.cpp
//       cutrace_amd/csrc/guard.cpp cutrace_amd/csrc/bvh.cpp -pthread
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scene_flatten.h"

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double u() { return (double)(next() >> 11) * 0x1p-53; }            // [0, 1)
  double u(double a, double b) { return a + (b - a) * u(); }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct V { float x, y, z; };
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }   // vector.hpp: left to right
V scale(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V mul(V a, V b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
V normalized(V a) { const float inv = 1.0f / sqrtf(dot(a, a)); return scale(a, inv); }
float smax(float a, float b) { return (a < b) ? b : a; }          // std::max's select
float ulps(float x, int k) { for (int i = 0; i < abs(k); i++) x = nextafterf(x, k > 0 ? INFINITY : -INFINITY); return x; }
bool is_zero_bits(float f) { return (bits(f) & 0x7FFFFFFFu) == 0u; }
bool is_neg_zero(float f) { return bits(f) == 0x80000000u; }

const float EXPS[7] = {0.0f, 0.5f, 1.0f, 2.0f, 200.0f, 1000.0f, 1e5f};

// a colour component: mostly ordinary, with every special value among them
float colour(Rng &R) {
  switch (R.below(24)) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return 0.5f;
    case 3: return -0.7f;
    case 4: return 0.2f;
    case 5: return 1.0f;
    case 6: return -1.0f;
    case 7: return INFINITY;
    case 8: return -INFINITY;
    case 9: return NAN;
    case 10: return 1e30f;
    case 11: return -3e38f;
    case 12: return from_bits(1u + R.below(0x7FFFFFu));                 // a denormal
    case 13: return -from_bits(1u + R.below(0x7FFFFFu));
    case 14: return (float)pow(2.0, R.u(38, 42));                       // either side of the bound
    case 15: return CTR_SHADE_BOUND;
    case 16: return nextafterf(CTR_SHADE_BOUND, INFINITY);
    default: return (float)R.u(-1.5, 1.5);
  }
}
V colour3(Rng &R) {
  if (R.below(8) == 0) return {0.5f, -0.7f, 0.2f};
  return {colour(R), colour(R), colour(R)};
}
// a unit vector, often along an axis (then the dots below are single products, and signed zeros survive)
V unit(Rng &R) {
  if (R.below(3) == 0) {
    const float s = R.below(2) ? 1.0f : -1.0f;
    const float z = R.below(2) ? 0.0f : -0.0f;
    switch (R.below(3)) { case 0: return {s, z, -z}; case 1: return {z, s, z}; default: return {-z, z, s}; }
  }
  for (;;) {
    const V v = {(float)R.u(-1, 1), (float)R.u(-1, 1), (float)R.u(-1, 1)};
    const float d = dot(v, v);
    if (d > 1e-3f && d <= 1.0f) return normalized(v);
  }
}
// a unit vector whose dot with n is `c` up to rounding: c * n + sqrt(1 - c^2) * (a direction perpendicular to n)
V at_cosine(Rng &R, V n, float c) {
  V t;
  for (;;) {
    const V r = unit(R);
    const float k = dot(r, n);
    t = add(r, scale(n, -k));
    if (dot(t, t) > 1e-4f) break;
  }
  t = normalized(t);
  const float s = sqrtf(smax(0.0f, 1.0f - c * c));
  return add(scale(n, c), scale(t, s));
}
// a cosine near where the predicate turns: exactly +-0, a denormal, a few ulp of rounding noise around 0, or anything
float cosine(Rng &R) {
  switch (R.below(10)) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return from_bits(1u + R.below(64u)) * (R.below(2) ? 1.0f : -1.0f);
    case 3: return (float)R.u(-4, 4) * 0x1p-24f;
    case 4: return (float)R.u(-4, 4) * 0x1p-20f;
    case 5: return (float)R.u(-1, 0);
    default: return (float)R.u(-1, 1);
  }
}

struct Mutations { bool no_neg_zero_guard = false, denormal_is_zero = false, no_bound = false; };

}  // namespace

int main(int argc, char **argv) {
  uint64_t cases = 20000000ull, seed = 1;
  Mutations mut;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--no-neg-zero-guard")) mut.no_neg_zero_guard = true;
    else if (!strcmp(argv[i], "--denormal-is-zero")) mut.denormal_is_zero = true;
    else if (!strcmp(argv[i], "--no-bound")) mut.no_bound = true;
    else if (argv[i][0] >= '0' && argv[i][0] <= '9') cases = strtoull(argv[i], nullptr, 10);
    else { fprintf(stderr, "dark_light_check: unknown argument %s\n", argv[i]); return 2; }
  }
  Rng R{seed * 0x2545F4914F6CDD1Dull + 99};
  uint64_t n_dark = 0, violations = 0, finite_mismatch = 0, n_facts = 0;
  uint64_t refused_neg_zero = 0, refused_denormal = 0, refused_bound = 0, refused_nonfinite = 0, fd_zero_n = 0, fs_zero_n = 0, near_zero = 0;
  uint64_t by_exp[7] = {0, 0, 0, 0, 0, 0, 0}, dark_by_exp[7] = {0, 0, 0, 0, 0, 0, 0}, fast_n = 0, neg_colour_dark = 0;
  for (uint64_t it = 0; it < cases; it++) {
    // ---- the scene of the case: one material, one light (shade_facts reads the records the launch would carry) ----
    DMat M{};
    DLight L{};
    const bool tame = R.below(4) != 0;  // most cases keep the colours ordinary, so that D is reached often
    auto col = [&]() -> float { return tame ? (R.below(6) == 0 ? (R.below(2) ? 0.0f : -0.0f) : (float)R.u(-1.5, 1.5)) : colour(R); };
    if (tame && R.below(6) == 0) { L.cx = 0.5f; L.cy = -0.7f; L.cz = 0.2f; } else { L.cx = col(); L.cy = col(); L.cz = col(); }
    if (!tame && R.below(4) == 0) { const V c = colour3(R); M.cx = c.x; M.cy = c.y; M.cz = c.z; } else { M.cx = col(); M.cy = col(); M.cz = col(); }
    M.specular = col();
    int ei = (int)R.below(8);
    M.phong_exp = ei < 7 ? EXPS[ei] : (float)pow(10.0, R.u(-1, 5));
    // what the facts must NOT look at
    M.reflexivity = R.below(16) == 0 ? NAN : 0.25f;
    M.transparency = 0.0f;
    if (R.below(16) == 0) { M.phong_exp = R.below(2) ? INFINITY : NAN; ei = 7; }
    L.type = 1u;
    L.vx = R.below(16) == 0 ? INFINITY : 1.0f; L.vy = 2.0f; L.vz = R.below(16) == 0 ? NAN : 3.0f;
    const uint32_t facts = shade_facts(&M, 1, &L, 1);
    const bool all_finite = std::isfinite(M.cx) && std::isfinite(M.cy) && std::isfinite(M.cz) && std::isfinite(M.specular) &&
                            std::isfinite(L.cx) && std::isfinite(L.cy) && std::isfinite(L.cz);
    if (((facts & 1u) != 0u) != all_finite) finite_mismatch++;
    const bool word = mut.no_bound ? (facts & 1u) != 0u : facts == 3u;
    if (word) n_facts++;

    // ---- the geometry of the pair: nn.nd and nn.h near zero on both sides ----
    const V nn = unit(R);
    const float c_d = cosine(R);
    const V nd = R.below(8) == 0 ? unit(R) : at_cosine(R, nn, c_d);
    V in_dn;
    if (R.below(3) == 0) {
      // the half vector at a chosen cosine to nn: in_dn = -(2 (nd.h) h - nd), the mirror image of nd in h, negated
      const V h = at_cosine(R, nn, cosine(R));
      const float k = 2.0f * dot(nd, h);
      in_dn = scale(add(scale(h, k), scale(nd, -1.0f)), -1.0f);
    } else in_dn = unit(R);
    const float fd = smax(0.0f, dot(nn, nd));
    const V hsum = add(scale(in_dn, -1.0f), nd);
    const V hv = normalized(hsum);
    float sx = smax(0.0f, dot(nn, hv));
    // (a specular factor inside the denormals, where only the exact exponent arithmetic reaches: x^e = 2^-(127..149))
    const bool want_denormal = R.below(6) == 0 && M.phong_exp >= 2.0f && std::isfinite(M.phong_exp);
    if (want_denormal) sx = (float)exp2(-R.u(126.5, 149.5) / (double)M.phong_exp);
    const bool fast = R.below(2) == 0;
    float fs;
    if (fast) fs = (M.phong_exp == 0.0f) ? 1.0f : exp2f(M.phong_exp * log2f(sx));
    else fs = (float)pow((double)sx, (double)M.phong_exp);  // f64, rounded once
    fast_n += fast;
    if (ei < 7) by_exp[ei]++;
    if (fabsf(dot(nn, nd)) < 0x1p-20f) near_zero++;

    // ---- `final` so far: ambient, then what earlier lights may have added ----
    const float ambient = R.below(5) == 0 ? -0.25f : (R.below(8) == 0 ? (R.below(2) ? -0.0f : 0.0f) : (float)R.u(-0.5, 1.0));
    V fin = scale(V{M.cx, M.cy, M.cz}, ambient);
    if (R.below(2) == 0) fin = add(fin, V{(float)R.u(-1, 2), (float)R.u(-1, 2), (float)R.u(-1, 2)});
    if (R.below(16) == 0) fin.y = -0.0f;

    // ---- the predicate, as the kernel evaluates it ----
    const bool fd_zero = is_zero_bits(fd);
    const bool fs_zero = mut.denormal_is_zero ? fabsf(fs) < FLT_MIN : is_zero_bits(fs);
    const bool guard = mut.no_neg_zero_guard || !(is_neg_zero(fin.x) || is_neg_zero(fin.y) || is_neg_zero(fin.z));
    fd_zero_n += fd_zero;
    fs_zero_n += fd_zero && fs_zero;
    if (fd_zero && is_zero_bits(fs)) {
      if (!(facts & 1u)) refused_nonfinite++;
      else if (!(facts & 2u)) refused_bound++;
      else if (is_neg_zero(fin.x) || is_neg_zero(fin.y) || is_neg_zero(fin.z)) refused_neg_zero++;
    }
    if (fd_zero && !is_zero_bits(fs) && fabsf(fs) < FLT_MIN) refused_denormal++;
    if (!(word && fd_zero && fs_zero && guard)) continue;
    n_dark++;
    if (ei < 7) dark_by_exp[ei]++;
    if (L.cx < 0 || L.cy < 0 || L.cz < 0 || M.cx < 0 || M.cy < 0 || M.cz < 0 || M.specular < 0) neg_colour_dark++;

    // ---- shading.hpp:86-94 with shadow_fac = 0 ----
    const V diffuse = {M.cx, M.cy, M.cz}, color = {L.cx, L.cy, L.cz};
    const V specular = scale(diffuse, M.specular);  // default_schema.hpp:328
    const V ld = mul(diffuse, color), ls = mul(specular, color);
    const V term = scale(add(scale(ld, fd), scale(ls, fs)), 1 - 0.0f);
    const V out = add(fin, term);
    if (bits(out.x) != bits(fin.x) || bits(out.y) != bits(fin.y) || bits(out.z) != bits(fin.z)) {
      if (violations < 5)
        fprintf(stderr, "violation: fin %a %a %a + term %a %a %a = %a %a %a (fd %a fs %a)\n", fin.x, fin.y, fin.z, term.x, term.y, term.z, out.x,
                out.y, out.z, fd, fs);
      violations++;
    }
  }
  printf("checked cases %llu dark %llu violations %llu finite_mismatch %llu facts_hold %llu fd_zero %llu fd_and_fs_zero %llu near_zero_cosines %llu "
         "refused_neg_zero %llu refused_denormal_fs %llu refused_bound %llu refused_nonfinite %llu negative_colour_dark %llu fast_pow %llu",
         (unsigned long long)cases, (unsigned long long)n_dark, (unsigned long long)violations, (unsigned long long)finite_mismatch,
         (unsigned long long)n_facts, (unsigned long long)fd_zero_n, (unsigned long long)fs_zero_n, (unsigned long long)near_zero,
         (unsigned long long)refused_neg_zero, (unsigned long long)refused_denormal, (unsigned long long)refused_bound,
         (unsigned long long)refused_nonfinite, (unsigned long long)neg_colour_dark, (unsigned long long)fast_n);
  for (int e = 0; e < 7; e++) printf(" exp%d %llu dark_exp%d %llu", e, (unsigned long long)by_exp[e], e, (unsigned long long)dark_by_exp[e]);
  printf("\n");
  return 0;
}
