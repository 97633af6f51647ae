// guard_scan.h — the plane scan of the guard of the BVH culling (guard.h): is a triangle's plane one that a probe lies in?
//
// A probe is a point rays emanate from or end at (an eye, its image in a flat mirror, a point light) or a sun direction.
// guard.cpp scans on the host at ctr_scene_create and ctr_scene_set_cameras, guard_scan.hip on the device after an edit of
// the lights, the materials or a mesh (include/cutrace_edit.h, cutrace_update.h).  Both include THIS text, as tri_record.h and
// mesh_refit.h are shared: every operation below is one correctly rounded f64 +, -, *, |x|, max or compare on either side,
// so both give the same bit per plane.  Compile with -ffp-contract=off (a contracted multiply-add rounds once where this
// text rounds twice); no division and no square root here: the host takes a sun's length once, when it builds the probe.
// scripts/scene_edit_check.cpp holds the host compilation against the loop guard.cpp had before the two were split.
#ifndef CUTRACE_AMD_GUARD_SCAN_H
#define CUTRACE_AMD_GUARD_SCAN_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "tri_record.h"  // CTR_HD, CTR_PLANE_DOUBLES: the plane record guard_plane writes

#define CTR_GUARD_TOL (1.0 / 131072.0)  // 2^-17: an order of magnitude above the rounding that matters (guard.h)

// 32 bytes, read by a whole wave at once (a scalar load on the device).  A list of probes holds its points first, then its
// suns: the answer is an OR over the probes, so their order is free, and two plain loops without a branch on the kind are what
// the host compiler vectorises (a record that carries its kind cost the host scan half of its speed).
struct GuardProbe {
  double x, y, z;  // the point, or the sun's direction as the light carries it (floats, widened)
  double len;      // a sun: the length of (x, y, z); a point: unused, 0
};

// q: one plane record (unit normal, a point of the plane, the triangle's extent); probes[0 .. n_points) are points,
// probes[n_points .. n) suns.  true: some point lies in the plane, or some sun is parallel to it, within CTR_GUARD_TOL.
// A zero normal is a zero-area triangle: alpha is exactly 0, never a hit.
CTR_HD inline bool plane_is_risky(const double *q, const GuardProbe *probes, uint32_t n_points, uint32_t n) {
  if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0) return false;
  bool hit = false;
  for (uint32_t i = 0; i < n_points; i++) {
    const GuardProbe &p = probes[i];
    const double dx = p.x - q[3], dy = p.y - q[4], dz = p.z - q[5];
    const double dist = fabs(dx * q[0] + dy * q[1] + dz * q[2]);
    const double scale = fmax(fmax(fabs(dx), fabs(dy)), fmax(fabs(dz), q[6]));
    if (dist <= CTR_GUARD_TOL * scale) hit = true;
  }
  for (uint32_t i = n_points; i < n; i++) {
    const GuardProbe &p = probes[i];
    if (p.len > 0.0 && fabs(p.x * q[0] + p.y * q[1] + p.z * q[2]) <= CTR_GUARD_TOL * p.len) hit = true;
  }
  return hit;
}

// The scan's result is one bit per plane of ONE flat array (all meshes' planes, FlatScene::guards order): bit (k & 63) of
// word (k >> 6) for plane k.  A wave of the kernel writes one word; the host half below writes and cuts the same words.
inline uint64_t guard_scan_words(uint64_t n_planes) { return (n_planes + 63u) / 64u; }

// the host compilation of the scan: the words the kernel writes for planes[0 .. n)
inline void guard_scan_host(const double *planes, uint64_t n, const GuardProbe *probes, uint32_t n_points, uint32_t n_probes, uint64_t *words) {
  for (uint64_t w = 0; w < guard_scan_words(n); w++) words[w] = 0;
  for (uint64_t k = 0; k < n; k++)
    if (plane_is_risky(planes + CTR_PLANE_DOUBLES * k, probes, n_points, n_probes)) words[k >> 6] |= (uint64_t)1 << (k & 63u);
}

// a mesh's range [begin, begin + count) of the flat array cut out of the words: its set planes, relative to `begin`, ascending
inline std::vector<uint32_t> guard_scan_cut(const uint64_t *words, uint64_t begin, uint32_t count) {
  std::vector<uint32_t> risky;
  for (uint64_t k = begin; k < begin + count;) {
    const uint64_t w = words[k >> 6] >> (k & 63u);  // the rest of this word, plane k at bit 0
    const uint64_t left = 64u - (k & 63u), end = begin + count;
    if (w)
      for (uint64_t b = 0; b < left && k + b < end; b++)
        if ((w >> b) & 1u) risky.push_back((uint32_t)(k + b - begin));
    k += left;
  }
  return risky;
}

// The launcher of guard_scan.hip: words[0 .. guard_scan_words(n)) of device memory receive the bits of the n planes at
// `planes` against the probes at `probes`, n_points points and then suns up to n_probes (device memory both).  Returns a hipError_t as int and queues its work
// on `stream`; it does not wait.
int ctr_launch_guard_scan(const double *planes, uint32_t n, const GuardProbe *probes, uint32_t n_points, uint32_t n_probes, uint64_t *words,
                          void *stream);

#endif
