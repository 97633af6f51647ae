// nearest_check.cpp — the host half of the nearest-point query (cutrace_amd/csrc/nearest_point.h), stand-alone:
//
//   g++ -std=c++17 -O2 -ffp-contract=off -pthread -Icutrace_amd/csrc -Iinclude -o nearest_check scripts/nearest_check.cpp
//   ./nearest_check            (a) (b) (c) below; ends with "all checks hold", status 0, when they do
//   ./nearest_check a|b|c      one part
//   ./nearest_check eval IN OUT   np_triangle of every 12-float row of IN (a, b, A, p) as 4 floats (d2, q) into OUT: what
//                              tests/test_nearest_cpu.py holds tests/nearest_ref.py to, bit for bit
// (tests/test_nearest_cpu.py builds and runs it; with -fsanitize=address,undefined it is the run of profiles/nearest/sanitizers.txt.)
//
// (a) np_triangle against a float64 brute force of ANOTHER algorithm (project onto the plane; outside the face, clamp onto the
//     three segments), on the record's triangle: random triangles and points, slivers, points on vertices, on edges, in the face
//     plane, far points.  Measures k = |distance - distance64| / (2^-24 * (distance64 + largest edge + |p - A|)) and holds it to
//     NP_K_BAR, four times the largest k this search has seen (DESIGN.md §28 has both numbers).
// (b) the cull: random trees over random triangle sets at scales 2^-20 .. 2^24, up to 2^18 scene sizes off the origin; points
//     random, on box faces and just outside them.  No box may have a margined bound (np_box_bound) above the computed d2 of a
//     triangle inside it.
// (c) the same search with every box shrunk inward by 2^-10 of its extent must REPORT violations: the search can see one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "nearest_point.h"

#define NP_K_BAR 8.0  // 4 x the measured 1.99 (part (a), the largest of every class)

namespace {

std::mt19937_64 rng(20260428);
double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
uint32_t pick(uint32_t n) { return (uint32_t)(rng() % n); }

struct D3 { double x, y, z; };
D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 operator*(D3 a, double f) { return {a.x * f, a.y * f, a.z * f}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(D3 a) { return sqrt(dot(a, a)); }

double seg_dist(D3 p, D3 a, D3 b) {
  const D3 e = b - a;
  const double ee = dot(e, e);
  double t = ee > 0.0 ? dot(p - a, e) / ee : 0.0;
  t = std::min(1.0, std::max(0.0, t));
  return len(p - (a + e * t));
}

// distance of p to the triangle (A, B, C) in float64: the foot on the plane when it lies inside all three edges, else the
// nearest of the three segments
double brute(D3 p, D3 A, D3 B, D3 C) {
  const D3 n = cross(B - A, C - A);
  const double nn = dot(n, n);
  if (nn > 0.0) {
    const double h = dot(p - A, n) / nn;
    const D3 f = p - n * h;
    if (dot(cross(B - A, f - A), n) >= 0.0 && dot(cross(C - B, f - B), n) >= 0.0 && dot(cross(A - C, f - C), n) >= 0.0)
      return fabs(dot(p - A, n)) / sqrt(nn);
  }
  return std::min(seg_dist(p, A, B), std::min(seg_dist(p, B, C), seg_dist(p, C, A)));
}

NpCand cand(const DTri &T, const ctr_vec3 &p) {
  return np_triangle(T.ab[0][0], T.ab[1][0], T.ab[2][0], T.ab[0][1], T.ab[1][1], T.ab[2][1], T.px, T.py, T.pz, p.x, p.y, p.z);
}

ctr_vec3 v3(double x, double y, double z) { ctr_vec3 v; v.x = (float)x; v.y = (float)y; v.z = (float)z; return v; }
ctr_vec3 rand_in(double r) { return v3(uni(-r, r), uni(-r, r), uni(-r, r)); }
D3 d3(const ctr_vec3 &v) { return {v.x, v.y, v.z}; }

// ---- (a) ----
const char *CLASSES[] = {"random", "sliver", "on a vertex", "on an edge", "in the face plane", "far"};
double k_of(const ctr_vec3 t[3], const ctr_vec3 &p, bool &nan) {
  DTri T;
  float gn[4];
  make_tri(t[0], t[1], t[2], 0, T, gn);
  const NpCand c = cand(T, p);
  // the record's triangle, exactly: A, A - a, A - b
  const D3 A = {T.px, T.py, T.pz};
  const D3 B = {(double)T.px - T.ab[0][0], (double)T.py - T.ab[1][0], (double)T.pz - T.ab[2][0]};
  const D3 Cc = {(double)T.px - T.ab[0][1], (double)T.py - T.ab[1][1], (double)T.pz - T.ab[2][1]};
  nan = !(c.d2 == c.d2);
  if (nan) return 0.0;
  const double want = brute(d3(p), A, B, Cc);
  const double edge = std::max(len(B - A), std::max(len(Cc - A), len(Cc - B)));
  const double scale = ldexp(1.0, -24) * (want + edge + len(d3(p) - A));
  return scale > 0.0 ? fabs((double)sqrtf(c.d2) - want) / scale : 0.0;
}

int part_a() {
  double kmax[6] = {0, 0, 0, 0, 0, 0};
  long cases = 0, nans = 0;
  for (int it = 0; it < 1200000; it++) {
    const int cls = it % 6;
    const double s = ldexp(1.0, (int)pick(41) - 20);  // the triangle's size, 2^-20 .. 2^20
    ctr_vec3 t[3] = {rand_in(s), rand_in(s), rand_in(s)};
    if (cls == 1) {  // sliver: the third corner on the line of the first two, pushed off it by 2^-4 .. 2^-20 of the edge
      const double f = uni(-0.5, 1.5), off = ldexp(1.0, -4 - (int)pick(17));
      const ctr_vec3 r = rand_in(s * off);
      t[2] = v3(t[0].x + f * ((double)t[1].x - t[0].x) + r.x, t[0].y + f * ((double)t[1].y - t[0].y) + r.y, t[0].z + f * ((double)t[1].z - t[0].z) + r.z);
    }
    ctr_vec3 p = rand_in(2.0 * s);
    const double u = uni(0, 1), w = uni(0, 1) * (1.0 - u);
    if (cls == 2) p = t[pick(3)];
    if (cls == 3) { const int e = pick(3); const ctr_vec3 &a = t[e], &b = t[(e + 1) % 3]; p = v3(a.x + u * ((double)b.x - a.x), a.y + u * ((double)b.y - a.y), a.z + u * ((double)b.z - a.z)); }
    if (cls == 4) {  // in the plane, inside the face or up to two edge lengths outside
      const double uu = pick(2) ? u : uni(-2, 3), ww = pick(2) ? w : uni(-2, 3);
      p = v3(t[0].x + uu * ((double)t[1].x - t[0].x) + ww * ((double)t[2].x - t[0].x), t[0].y + uu * ((double)t[1].y - t[0].y) + ww * ((double)t[2].y - t[0].y),
             t[0].z + uu * ((double)t[1].z - t[0].z) + ww * ((double)t[2].z - t[0].z));
    }
    if (cls == 5) { const double far = ldexp(1.0, 3 + (int)pick(22)); p = rand_in(s * far); }  // 2^3 .. 2^24 triangle sizes away
    bool nan;
    const double k = k_of(t, p, nan);
    cases++;
    nans += nan;
    kmax[cls] = std::max(kmax[cls], k);
  }
  double k = 0;
  for (int c = 0; c < 6; c++) {
    printf("a: %-18s k_max %.3f\n", CLASSES[c], kmax[c]);
    k = std::max(k, kmax[c]);
  }
  printf("a: cases %ld nan %ld k_max %.3f bar %.1f\n", cases, nans, k, (double)NP_K_BAR);
  return (k <= NP_K_BAR && nans == 0) ? 0 : 1;
}

// ---- (b), (c) ----
struct Set {
  std::vector<ctr_triangle> file;
  std::vector<DTri> rec;
  float lo[3], hi[3];
};
void bounds(const std::vector<ctr_triangle> &t, const uint32_t *idx, size_t n, float *lo, float *hi) {
  for (int a = 0; a < 3; a++) { lo[a] = INFINITY; hi[a] = -INFINITY; }
  for (size_t k = 0; k < n; k++) {
    const ctr_vec3 *v[3] = {&t[idx[k]].p1, &t[idx[k]].p2, &t[idx[k]].p3};
    for (int c = 0; c < 3; c++)
      for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], (&v[c]->x)[a]); hi[a] = fmaxf(hi[a], (&v[c]->x)[a]); }
  }
}

struct Tally { long boxes = 0, pairs = 0, violations = 0; double worst = 0; };

// one box of a tree (the triangles idx[0 .. n)) against a handful of points, then its two halves along a random axis
void visit(const Set &S, uint32_t *idx, size_t n, float shrink, Tally &T) {
  float lo[3], hi[3];
  bounds(S.file, idx, n, lo, hi);
  float blo[3], bhi[3];
  for (int a = 0; a < 3; a++) { const float e = (hi[a] - lo[a]) * shrink; blo[a] = lo[a] + e; bhi[a] = hi[a] - e; }
  T.boxes++;
  float ext = 0;
  for (int a = 0; a < 3; a++) ext = fmaxf(ext, S.hi[a] - S.lo[a]);
  for (int q = 0; q < 12; q++) {
    float p[3];
    for (int a = 0; a < 3; a++) {
      const uint32_t how = pick(6);
      const float e = hi[a] - lo[a];
      if (how == 0) p[a] = (float)uni(lo[a], hi[a]);                               // inside the slab
      else if (how == 1) p[a] = pick(2) ? lo[a] : hi[a];                           // on a face
      else if (how == 2) p[a] = pick(2) ? nextafterf(lo[a], -INFINITY) : nextafterf(hi[a], INFINITY);  // one ulp outside
      else if (how == 3) p[a] = (float)(pick(2) ? lo[a] - uni(0, 1) * e * ldexp(1.0, -(int)pick(24)) : hi[a] + uni(0, 1) * e * ldexp(1.0, -(int)pick(24)));
      else if (how == 4) p[a] = (float)uni(S.lo[a] - ext, S.hi[a] + ext);          // about the mesh
      else p[a] = (float)(0.5 * ((double)S.lo[a] + S.hi[a]) + uni(-1, 1) * ext * ldexp(1.0, (int)pick(12)));  // far
    }
    const float mw = np_margin(p[0], p[1], p[2], S.lo[0], S.lo[1], S.lo[2], S.hi[0], S.hi[1], S.hi[2]);
    const float b = np_box_bound(blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], p[0], p[1], p[2], mw);
    const size_t step = n > 64 ? n / 64 : 1;
    for (size_t k = 0; k < n; k += step) {
      ctr_vec3 pp; pp.x = p[0]; pp.y = p[1]; pp.z = p[2];
      const NpCand c = cand(S.rec[idx[k]], pp);
      T.pairs++;
      if (b > c.d2) {  // the walk would have dropped this triangle although it can still win or tie
        T.violations++;
        T.worst = std::max(T.worst, ((double)b - c.d2) / (double)b);
      }
    }
  }
  if (n <= 2) return;
  const int axis = pick(3);
  auto centre = [&](uint32_t i) { const ctr_triangle &t = S.file[i]; return (&t.p1.x)[axis] + (&t.p2.x)[axis] + (&t.p3.x)[axis]; };
  const size_t half = 1 + pick((uint32_t)n - 1);
  std::nth_element(idx, idx + half, idx + n, [&](uint32_t x, uint32_t y) { return centre(x) < centre(y); });
  visit(S, idx, half, shrink, T);
  visit(S, idx + half, n - half, shrink, T);
}

Tally search(float shrink, int sets) {
  Tally T;
  const int offs[] = {-1, 10, 14, 18};
  for (int s = 0; s < sets; s++) {
    const int k = (int)pick(45) - 20;  // 2^-20 .. 2^24
    const int oe = offs[pick(4)];
    const double scale = ldexp(1.0, k);
    const double off[3] = {oe < 0 ? 0.0 : scale * ldexp(1.0, oe), oe < 0 ? 0.0 : -0.75 * scale * ldexp(1.0, oe), oe < 0 ? 0.0 : 0.5 * scale * ldexp(1.0, oe)};
    Set S;
    const size_t n = 8 + pick(120);
    const double tri = ldexp(1.0, -(int)pick(8));  // triangle size relative to the set's
    for (size_t q = 0; q < n; q++) {
      const double c[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
      ctr_triangle t;
      ctr_vec3 *v[3] = {&t.p1, &t.p2, &t.p3};
      for (int j = 0; j < 3; j++)
        *v[j] = v3((float)((c[0] + uni(-tri, tri)) * scale) + (float)off[0], (float)((c[1] + uni(-tri, tri)) * scale) + (float)off[1],
                   (float)((c[2] + uni(-tri, tri)) * scale) + (float)off[2]);
      S.file.push_back(t);
      DTri T1;
      float gn[4];
      make_tri(t.p1, t.p2, t.p3, (uint32_t)q, T1, gn);
      S.rec.push_back(T1);
    }
    std::vector<uint32_t> idx(n);
    for (size_t q = 0; q < n; q++) idx[q] = (uint32_t)q;
    bounds(S.file, idx.data(), n, S.lo, S.hi);
    visit(S, idx.data(), n, shrink, T);
  }
  return T;
}

int part_b() {
  const Tally T = search(0.0f, 1500);
  printf("b: boxes %ld pairs %ld violations %ld\n", T.boxes, T.pairs, T.violations);
  return T.violations == 0 ? 0 : 1;
}

int part_c() {
  const Tally T = search(0x1p-10f, 300);
  printf("c: boxes %ld pairs %ld violations %ld (boxes shrunk by 2^-10 of their extent)\n", T.boxes, T.pairs, T.violations);
  return T.violations > 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  const char *which = argc > 1 ? argv[1] : "abc";
  if (argc == 4 && !strcmp(which, "eval")) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    float r[12];
    while (fread(r, sizeof(float), 12, in) == 12) {
      const NpCand c = np_triangle(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11]);
      const float o[4] = {c.d2, c.qx, c.qy, c.qz};
      if (fwrite(o, sizeof(float), 4, out) != 4) return 2;
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
  }
  int bad = 0;
  if (strchr(which, 'a')) bad |= part_a();
  if (strchr(which, 'b')) bad |= part_b();
  if (strchr(which, 'c')) bad |= part_c();
  if (!bad) printf("all checks hold\n");
  return bad;
}
