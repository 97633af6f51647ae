// nearest_point.h — the definition of ctr_nearest_points (include/cutrace_nearest.h): for a query point p, the candidate
// (d2, q) of ONE object — d2 the squared distance, q the closest point on the object — and the lower bound of a box that
// the mesh walk culls with.
//
// ray_nearest.hip evaluates it on the device, scripts/nearest_check.cpp on the host, tests/nearest_ref.py restates it in NumPy.
// All three follow THIS text: every operation below is a single correctly rounded f32 +, -, *, /, sqrt or compare (a select
// on a compare, never fminf / fmaxf: those leave the sign of a zero and the fate of a NaN to the platform), in the order
// written — but for np_dop, three correctly rounded f64 operations and a narrowing.  Compile with -ffp-contract=off.  A dot product is (x*x' + y*y') + z*z'.  DESIGN.md §28.
//
// THE ANSWER for a point is the lexicographic minimum of (d2, object index) over the objects the query admits, inside a mesh
// of (d2, file index) — the tie rules ray_cast has for t — over the candidates that COUNT: d2 <= lim2 and d2 < +inf, with
// lim2 = max_dist * max_dist.  A NaN compares false, so a NaN candidate never counts; a point with a NaN or an infinity in
// it has no finite d2 with any object and gets the miss values.
#ifndef CUTRACE_AMD_NEAREST_POINT_H
#define CUTRACE_AMD_NEAREST_POINT_H

#include <math.h>
#include <stdint.h>

#include "tri_record.h"  // CTR_HD

struct NpCand {
  float d2;          // squared distance of p to the object
  float qx, qy, qz;  // the closest point
};

// a*b - c*d with ONE rounding that matters: both products are exact in f64 (24 + 24 bits), their difference is rounded to f64
// and then to f32.  The one place where f32 alone will not do: the normal of a thin triangle is the difference of nearly
// equal products.  (Defined through f64, not fmaf: NumPy has no fused multiply-add, and f64 +, -, * are the same everywhere.)
CTR_HD inline float np_dop(float a, float b, float c, float d) { return (float)((double)a * (double)b - (double)c * (double)d); }

// TRIANGLE, from its DTri record alone: corner A = (Ax, Ay, Az) = the record's (px, py, pz), edges AB = -a and AC = -b of
// the stored a = p2 - p1, b = p2 - p3.  The triangle is the RECORD's: A, B = A + AB, C = A + AC (B may differ from the file's p1
// in the last bit).  Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5) — vertex regions first, then edge
// regions, then the face, in his order and with his tests — with two changes that keep a sliver's and a far point's answer:
//   - the barycentric products va, vb, vc, of which only the SIGNS are used (is the foot of p on the inner side of an edge?),
//     are formed as (n x edge).(p - corner) with the normal n = AB x AC by np_dop.  Their textbook forms d1*d4 - d3*d2 ...
//     (and aa*d2 - g*d1 ... from the Gram constants) are differences of products of size |edge|^3 |AP| that decide a length of
//     |n| |edge| x (distance to the edge line): the sign is lost 1 / sin(thinnest angle) times sooner;
//   - in the face region the closest point is the foot of the perpendicular, q = p - s * nh with nh = n / |n| and
//     s = nh.AP, d2 = s*s (np_plane's text), not A + v*AB + w*AC with v = vb / (va + vb + vc): those quotients carry
//     the same cancellation, and along a sliver they move q by |edge| / sin^2 x 2^-24.
// With AP = p - A:  d1 = AB.AP, d2 = AC.AP, d3 = AB.BP = d1 - AB.AB, d6 = AC.CP = d2 - AC.AC.  In a vertex or edge region q = A + t with t = v*AB + w*AC, 0 <= v, w, v + w <= 1, and
// d2 = |AP - t|^2: the same vector as p - q, formed without the detour over the coordinates' own magnitude, so that a scene
// far off the origin keeps the distance's precision (q itself cannot).
// What the cull of the mesh walk rests on (np_box_bound): q is a point of the record's triangle to within the rounding of its
// terms, or — the face — a point of its plane whose distance cannot exceed the triangle's by more than the rounding of the edge
// tests, a few 2^-24 |AP|.  A record with a zero edge or zero area that reaches a 0/0 gives a NaN d2 and so no candidate.
CTR_HD inline NpCand np_triangle(float ax, float ay, float az, float bx, float by, float bz, float Ax, float Ay, float Az,
                                 float px, float py, float pz) {
  const float abx = -ax, aby = -ay, abz = -az, acx = -bx, acy = -by, acz = -bz;
  const float apx = px - Ax, apy = py - Ay, apz = pz - Az;
  const float aa = (abx * abx + aby * aby) + abz * abz;
  const float cc = (acx * acx + acy * acy) + acz * acz;
  const float d1 = (abx * apx + aby * apy) + abz * apz;
  const float d2 = (acx * apx + acy * apy) + acz * apz;
  const float d3 = d1 - aa, d6 = d2 - cc;
  // along BC the two projections are taken on BC itself: e1 = BC.BP (Ericson's d4 - d3), e2 = BC.PC (his d5 - d6), with
  // BC = AC - AB, BP = AP - AB, PC = AC - AP; as differences of d's a short BC would drown in the rounding of the long edges
  const float cx = acx - abx, cy = acy - aby, cz = acz - abz;
  const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
  const float e1 = (cx * bpx + cy * bpy) + cz * bpz;
  const float e2 = (cx * (acx - apx) + cy * (acy - apy)) + cz * (acz - apz);
  NpCand c;
  float v, w;
  if (d1 <= 0.0f && d2 <= 0.0f) {  // vertex A
    v = 0.0f; w = 0.0f;
  } else if (d3 >= 0.0f && e1 <= 0.0f) {  // vertex B
    v = 1.0f; w = 0.0f;
  } else {
    const float nx = np_dop(aby, acz, abz, acy), ny = np_dop(abz, acx, abx, acz), nz = np_dop(abx, acy, aby, acx);
    // vc = (n x AB).AP
    const float vc = ((ny * abz - nz * aby) * apx + (nz * abx - nx * abz) * apy) + (nx * aby - ny * abx) * apz;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {  // edge AB
      v = d1 / (d1 - d3); w = 0.0f;
    } else if (d6 >= 0.0f && e2 <= 0.0f) {  // vertex C
      v = 0.0f; w = 1.0f;
    } else {
      // vb = (AC x n).AP
      const float vb = ((acy * nz - acz * ny) * apx + (acz * nx - acx * nz) * apy) + (acx * ny - acy * nx) * apz;
      if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {  // edge AC
        v = 0.0f; w = d2 / (d2 - d6);
      } else {
        // va = (n x BC).BP
        const float va = ((ny * cz - nz * cy) * bpx + (nz * cx - nx * cz) * bpy) + (nx * cy - ny * cx) * bpz;
        if (va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {  // edge BC
          w = e1 / (e1 + e2); v = 1.0f - w;
        } else {  // the face: the foot of the perpendicular
          const float f = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
          const float hx = nx * f, hy = ny * f, hz = nz * f;
          const float s = (apx * hx + apy * hy) + apz * hz;
          c.d2 = s * s;
          c.qx = px - s * hx; c.qy = py - s * hy; c.qz = pz - s * hz;
          return c;
        }
      }
    }
  }
  const float tx = v * abx + w * acx, ty = v * aby + w * acy, tz = v * abz + w * acz;
  const float rx = apx - tx, ry = apy - ty, rz = apz - tz;
  c.d2 = (rx * rx + ry * ry) + rz * rz;
  c.qx = Ax + tx; c.qy = Ay + ty; c.qz = Az + tz;
  return c;
}

// SPHERE of centre c and radius R: v = p - c, len = sqrtf(v.v), s = len - |R|, d2 = s*s, q = c + v * (|R| / len); for
// len == 0 (the centre itself) q = (c.x + |R|, c.y, c.z).  (d2 is NOT |p - q|^2 here: s*s is the distance's own rounding.)
CTR_HD inline NpCand np_sphere(float cx, float cy, float cz, float R, float px, float py, float pz) {
  const float vx = px - cx, vy = py - cy, vz = pz - cz;
  const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
  const float r = R < 0.0f ? -R : R;
  const float s = len - r;
  NpCand c;
  c.d2 = s * s;
  if (len == 0.0f) {
    c.qx = cx + r; c.qy = cy; c.qz = cz;
  } else {
    const float k = r / len;
    c.qx = cx + vx * k; c.qy = cy + vy * k; c.qz = cz + vz * k;
  }
  return c;
}

// PLANE through p0 with normal n: nh = n * (1 / |n|), s = (p - p0).nh, d2 = s*s, q = p - s * nh.  A zero normal gives NaN.
CTR_HD inline NpCand np_plane(float x0, float y0, float z0, float nx, float ny, float nz, float px, float py, float pz) {
  const float f = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
  const float hx = nx * f, hy = ny * f, hz = nz * f;
  const float s = ((px - x0) * hx + (py - y0) * hy) + (pz - z0) * hz;
  NpCand c;
  c.d2 = s * s;
  c.qx = px - s * hx; c.qy = py - s * hy; c.qz = pz - s * hz;
  return c;
}

// does a candidate count against the limit `lim2`?
CTR_HD inline bool np_counts(float d2, float lim2) { return d2 <= lim2 && d2 < INFINITY; }

// ---- the cull of the mesh walk ----
// The margin of one (point, mesh) pair: mw = 2^-19 * G, with G the largest |coordinate difference| between p and a corner of
// the MESH's box (bmin, bmax).  DESIGN.md §28 derives it: a computed d2 is the squared distance to a point of its file triangle
// to within 2^-24 * 12.2 G, and the roundings of d2 and of the bound itself add less than 2^-24 * 7 G.
CTR_HD inline float np_margin(float px, float py, float pz, float lx, float ly, float lz, float hx, float hy, float hz) {
  float G = 0.0f, t;
  t = lx - px; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  t = hx - px; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  t = ly - py; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  t = hy - py; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  t = lz - pz; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  t = hz - pz; t = t < 0.0f ? -t : t; G = t > G ? t : G;
  return G * 0x1p-18f;
}

// one axis of the bound: max(lo - p, p - hi, 0), less the margin, not below 0
CTR_HD inline float np_axis_bound(float lo, float hi, float p, float mw) {
  const float a = lo - p, b = p - hi;
  float t = a > b ? a : b;
  t = t - mw;
  return t > 0.0f ? t : 0.0f;
}

// The margined lower bound of the box (lo, hi): no triangle whose file vertices lie in the box has a COMPUTED d2 below it.  A
// child (or a mesh) is dropped only when this bound is strictly above the limit: an equal d2 is still found.
CTR_HD inline float np_box_bound(float lx, float ly, float lz, float hx, float hy, float hz, float px, float py, float pz, float mw) {
  const float tx = np_axis_bound(lx, hx, px, mw), ty = np_axis_bound(ly, hy, py, mw), tz = np_axis_bound(lz, hz, pz, mw);
  return (tx * tx + ty * ty) + tz * tz;
}

#endif
