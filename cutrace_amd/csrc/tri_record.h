// tri_record.h — what the scene keeps of ONE triangle, computed from its three vertices: the DTri record and the geometric
// normal (scene_device.h), and the plane record of the guard (guard.h, MeshGuard::planes).
//
// scene_flatten.cpp computes them on the host at ctr_scene_create, mesh_update.hip on the device at ctr_scene_update_mesh
// (include/cutrace_update.h).  Both include THIS text, so that an updated handle holds the bytes a fresh one would: every
// operation below is a single correctly rounded +, -, *, /, sqrt, min, max or |x| in f32 or f64 on either side (DESIGN.md §4
// "Numerics").  Compile with -ffp-contract=off: a contracted multiply-add rounds once where the reference rounds twice.
// scripts/mesh_update_check.cpp holds the host compilation of this header against flatten_scene byte for byte.
#ifndef CUTRACE_AMD_TRI_RECORD_H
#define CUTRACE_AMD_TRI_RECORD_H

#include <math.h>
#include <stdint.h>

#include "cutrace_amd.h"
#include "scene_device.h"

#ifdef __HIP__
#define CTR_HD __host__ __device__
#else
#define CTR_HD
#endif

#define CTR_TRI_KAPPA (1.0f / 16384.0f)  // prefilter slack factor 2^-14 (≈1000 ulp), see DESIGN.md
#define CTR_PLANE_DOUBLES 7              // per guard record: unit normal (3), a point of the plane (3), extent

// the DTri record of triangle (p1, p2, p3) with tie-break key `orig`, and its geometric normal (4 floats)
CTR_HD inline void make_tri(const ctr_vec3 &p1, const ctr_vec3 &p2, const ctr_vec3 &p3, uint32_t orig, DTri &T, float *gn) {
  const float ax = p2.x - p1.x, ay = p2.y - p1.y, az = p2.z - p1.z;  // a = p2 - p1, b = p2 - p3: default_schema.hpp:58
  const float bx = p2.x - p3.x, by = p2.y - p3.y, bz = p2.z - p3.z;
  T.ab[0][0] = ax; T.ab[1][0] = ay; T.ab[2][0] = az;
  T.ab[0][1] = bx; T.ab[1][1] = by; T.ab[2][1] = bz;
  T.px = p2.x; T.py = p2.y; T.pz = p2.z;
  T.nx = ay * bz - az * by;  // a x b (prefilter only)
  T.ny = az * bx - ax * bz;
  T.nz = ax * by - ay * bx;
  float emax = 0.f;
  emax = fmaxf(emax, fabsf(ax)); emax = fmaxf(emax, fabsf(ay)); emax = fmaxf(emax, fabsf(az));
  emax = fmaxf(emax, fabsf(bx)); emax = fmaxf(emax, fabsf(by)); emax = fmaxf(emax, fabsf(bz));
  T.ke = CTR_TRI_KAPPA * emax;
  T.ke2 = CTR_TRI_KAPPA * emax * emax;
  T.orig = orig;
  T.pad1 = 0.f;
  // default_schema.hpp:72: -1.0f * (p2 - p3).cross(p1 - p3).normalized()
  const float ux = p1.x - p3.x, uy = p1.y - p3.y, uz = p1.z - p3.z;
  const float cx = by * uz - bz * uy, cy = bz * ux - bx * uz, cz = bx * uy - by * ux;
  const float nrm = sqrtf(cx * cx + cy * cy + cz * cz);
  const float f = 1.0f / nrm;
  gn[0] = -1.0f * (f * cx);
  gn[1] = -1.0f * (f * cy);
  gn[2] = -1.0f * (f * cz);
  gn[3] = 0.f;
}

// the guard's record of the same triangle: its plane in double precision
CTR_HD inline void guard_plane(const ctr_vec3 &p1, const ctr_vec3 &p2, const ctr_vec3 &p3, double *q) {
  const double ax = (double)p2.x - p1.x, ay = (double)p2.y - p1.y, az = (double)p2.z - p1.z;
  const double bx = (double)p2.x - p3.x, by = (double)p2.y - p3.y, bz = (double)p2.z - p3.z;
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  if (len > 0.0) { q[0] = nx / len; q[1] = ny / len; q[2] = nz / len; } else { q[0] = q[1] = q[2] = 0.0; }
  q[3] = p2.x; q[4] = p2.y; q[5] = p2.z;
  q[6] = fmax(fmax(fmax(fabs(ax), fabs(ay)), fabs(az)), fmax(fmax(fabs(bx), fabs(by)), fabs(bz)));
}

#endif
