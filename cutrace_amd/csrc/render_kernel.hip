// render_kernel.hip — the per-pixel ray-cast + shading kernel for gfx950 (MI355X).
//
// What it replaces (reference, file:line):
//   render_kernel            inc/kernel.hpp:35-60
//   ray_cast                 inc/ray_cast.hpp:29-55
//   shadow_intensity/phong/ray_color   inc/shading.hpp:22-154
//   triangle/mesh/plane/sphere::intersect, lights, material, cam::get_ray
//                            inc/default_schema.hpp:22-399
//
// Design (MI355X-first, not a translation; the measurements behind each choice are in DESIGN.md):
//  * one lane = one pixel, one wave = an 8x8 pixel tile, one wave per workgroup.  The 64 rays of
//    a wave are spatially coherent and the scene is tiny and read-only, so EVERY scene read in the
//    hot loops has a wave-uniform address: planes, objects, BVH nodes and triangles are fetched
//    with scalar loads (one 64-byte record = one s_load_dwordx16) into SGPRs and feed the VALU as
//    scalar operands — no VGPRs, no LDS bandwidth, no bank conflicts.  (Measured, scripts/valu_issue.hip:
//    a VALU instruction with an SGPR operand issues at half rate, 4.1 cycles per wave64 instruction
//    against 2.2 — still the cheapest way to get a wave-uniform record to the lanes; a packed
//    instruction with an SGPR-PAIR operand does two such operations in the same 4.1 cycles, which is
//    why nodes, planes and triangles store their coordinates as aligned pairs.)
//  * the recursion of ray_color (template depth `bounces`) becomes an explicit per-lane state
//    machine: every trip of the outer loop performs exactly ONE nearest-hit cast for every live
//    lane, whatever that lane needs it for (primary, reflection, pass-through or a shadow-loop
//    iteration).  The expensive part (plane / object / BVH / triangle loops) is always executed by
//    a converged wave; only the cheap continuation logic diverges.  Suspended activations live in
//    an LDS stack [frame][field][lane] (4 dwords per frame); no scratch memory in the default build.
//  * hot-loop conditions are 64-bit lane masks (v_cmp into SGPR pairs, combined on the scalar
//    unit), not per-lane booleans.
//  * per mesh: the reference's AABB test decided with 1-ulp reciprocals except on borderline lanes;
//    a four-wide BVH (a node holds its four children's boxes, wave-uniform stack in the lanes of one
//    VGPR) walked by the whole wave, two child boxes per packed FMA; triangles whose plane contains an
//    eye or a light are additionally handed to every lane (guard records: the one regime where culling
//    could differ from the linear walk, ctr_scene.cpp refresh_linear_meshes); per triangle a
//    conservative FMA prefilter for the whole wave (barycentrics, then — only if a lane survives —
//    the ray parameter), then the reference's exact Cramer/determinant test
//    (default_schema.hpp:57-78) in the reference's operation order for surviving lanes, its three
//    IEEE divisions performed only where a 1-ulp reciprocal cannot decide.  Every shortcut acts
//    only on "certainly" (margins above the rounding of both evaluations), so results are identical
//    to the reference's linear walk (ties broken by file order).
//  * shadow rays stop at the first occluder when no material is transparent.
//  * the duplicated primary cast (kernel.hpp:52 + shading.hpp:123) is done once.
//  * arguments that only the continuation or the start of a cast needs are re-read from the kernarg
//    segment instead of living in SGPRs across the inner loops (no spill reloads by v_readlane); the
//    build avoids SLP vectorisation (compiler-made v_pk_* cost more in shuffles than they save).
//  * two builds of the default variant: 85 VGPRs = 5 waves per SIMD, and (KV_OCC6) 80 VGPRs = 6 waves, picked for scenes
//    with >= 1000 mesh triangles: five cold dwords of shading state live in one 1280-byte LDS granule behind the wave's
//    stack instead (PARK), mode and stack depth share a register, lane-derived addresses are recomputed from v_mbcnt.
//    No instantiation uses scratch memory.
//
// Numerics: compiled with -ffp-contract=off; +,-,*,/ and sqrt are IEEE correctly rounded on gfx950,
// so every geometric quantity (depth, hit, normal, which object is hit) is bit-identical to the
// reference's headers COMPILED FOR THE HOST — std::min/max select semantics for the unqualified min/max
// of the device code, no FMA contraction.  That, not a CUDA build (fminf/fmaxf-like overloads, --fmad),
// is the parity target; profiles/r02/cuda_minmax_gap.txt counts what the difference touches.
// The specular term — the half vector's normalisation and pow() — uses
// v_rsq_f32 and exp2(e*log2(x)) in f32 by default (colour within 3e-6 of the reference) or IEEE
// sqrt/division and f64 pow rounded once (CTR_VAR_EXACT_POW: the correctly rounded power, which glibc's powf is for all
// but about one argument in a thousand — there the reference's colour is the neighbouring float); it only
// feeds the colour.  Texture coordinates (atan2/asin, uv_for)
// are never produced: the only material type ignores them (default_schema.hpp:326-340).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "cutrace_amd.h"
#include "scene_device.h"
#include "bvh.h"
#include "kernel_choice.h"
#include "tile_order.h"
#include "tile_shape.h"
#include "vec3.h"

#define CADDR __attribute__((address_space(4)))
#define BALLOT(p) __builtin_amdgcn_ballot_w64(p)
#define HIDE_UNIFORM(x) asm volatile("" : "+v"(x))  /* make a wave-uniform index look per-lane: vector load */
#define PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))  /* opaque to LICM / speculation */
#define INVB(m) __builtin_amdgcn_inverse_ballot_w64(m)   /* wave-uniform lane mask -> per-lane predicate */
#define FCMP(a, b, pred) __builtin_amdgcn_fcmpf((a), (b), (pred))  /* v_cmp straight into a lane mask */
enum { FC_OEQ = 1, FC_OGT = 2, FC_OGE = 3, FC_OLT = 4, FC_OLE = 5 };  /* LLVM FCmp predicate numbers */
#define TL_NONE 0x7FFFFFFFu                                        /* "no more top-level items" */

// v_writelane_b32 with a wave-uniform value and lane select: this clang has no __builtin for it, so the
// LLVM intrinsic is bound by name (the compiler then routes the lane select through M0 by itself)
extern "C" __device__ uint32_t ctr_writelane(uint32_t value, uint32_t lane, uint32_t old) __asm("llvm.amdgcn.writelane.i32");

namespace {

#if defined(CTR_PROFILE)
__device__ unsigned int g_prof[256];  // executions of the CTR_MARK segments, summed over the waves of every launch ([128..255]: the shadow copy of a phased build)
#endif

// ---- how many lanes are alive (KV_STATS builds only; read by ctr_debug_lane_stats) ----
// A lane is one pixel for the pixel's whole life, and every trip of the kernel's loop casts one ray for every lane that
// still needs one — so lanes whose pixel is finished, or whose recursion is shallower than their neighbours', idle while
// the wave goes on (shading.hpp:126-150 is what diverges).  Counted per trip, split by what the lane casts for and how
// deep its recursion is:
//   [0..15]  lanes casting a radiance ray at recursion depth d (d = 0: the primary ray), summed over the trips
//   [16..31] lanes casting a shadow ray for a hit at depth d
//   [32..47] trips in which at least one lane casts a radiance ray at depth d;   [48..63] the same for shadow rays
//   [64..71] trips by the number of live lanes: 1-8, 9-16, ..., 57-64
//   [72] trips, [73] live lanes summed over the trips, [74] waves, [75] lanes inside the image summed over the waves,
//   [76] trips in which the live lanes cast for more than one (kind, depth)
//   [80] shadow wave casts that reach the mesh phase with live lanes, [81] those whose live lanes all start on a plane / sphere (not on a
//        mesh or triangle), [82] those of [81] in which no lane met an occluder in the mesh phase — what a perfect per-light occluder-distance
//        map could skip (built, measured and removed in round 4: those are the cheap casts, profiles/r04/exp_occluder_map.txt) —, [83] those of [80] in which no lane met an occluder in the mesh phase, whatever the receivers
//   [77] casts the merged walk handed back to the two-level walk (a mesh's AABB test failed for a lane the walk had decided,
//        or a mesh's nearest valid t equalled min_t), [78] casts that went through the merged walk
//   [88] any-hit shadow trips (trips with a live shadow lane, any-hit builds), [89] those that skipped their plane tests
//        ("room-safe lanes" in the kernel)
//   [90] (lane, light) pairs whose shadow cast cannot change the pixel ("dark lights" in the kernel; any-hit builds, launches whose
//        scene head carries the dark-skip word), [91] shadow trips whose live lanes are all such, [92] mesh entries of trips with
//        at least one such lane
__device__ unsigned long long g_lane_stats[96];

// ---- execution profile of the source's straight-line segments (scripts/dynamic_mix.py) ----
// CTR_MARK(n) opens segment n.  -DCTR_MARKS: a comment in the ISA, from which the segment's instructions are counted;
// -DCTR_PROFILE: a counter of how often a wave runs the segment — one global atomic add by lane 0 with EXEC forced
// to that lane and restored, so a segment inside divergent code counts once per wave that reaches it, whichever
// lanes are live; otherwise nothing.  The id is n + ctr_mark_base: zero here, and shadowed by a constant of the same name
// inside the shadow copy of a phased build's trip ("Phased builds" below), whose segments so get ids of their own (128 + n).
[[maybe_unused]] constexpr int ctr_mark_base = 0;
[[maybe_unused]] constexpr bool ctr_mark_fence = false;
#if defined(CTR_PROFILE)
#define CTR_MARK(n)                                                                                                    \
do {                                                                                                                 \
  unsigned long long pm_x;                                                                                           \
  uint32_t pm_a, pm_b;                                                                                               \
  asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 1\n\t"                    \
               "global_atomic_add %1, %2, %3 offset:%4\n\ts_mov_b64 exec, %0"                                         \
               : "=&s"(pm_x), "=&v"(pm_a), "=&v"(pm_b)                                                               \
               : "s"(g_prof), "n"(4 * ((n) + ctr_mark_base))                                                       \
               : "memory");                                                                                          \
} while (0)
#elif defined(CTR_MARKS)
#define CTR_MARK(n) asm volatile("; CTR_MARK %0" ::"n"((n) + ctr_mark_base))
#else
// (no profile: nothing — except in the copies of a phased build's trip, where every mark is an empty volatile statement the
//  optimiser does not move code across: with two inlined trips it otherwise merges and reorders the continuation's now
//  straight-line paths until the 6-wave builds spill to scratch — 80 VGPRs and 8 to 16 bytes of scratch without the fences,
//  67 to 73 VGPRs and fewer instructions with them, profiles/r09/phase_static.txt.  ctr_mark_fence is false here and shadowed,
//  like ctr_mark_base, inside those copies; a mark of any other code compiles to nothing, as before.)
// (an `if constexpr` with its own else, so that an `else` after a mark can never bind to it; wrapped in do { } while (0) the
//  empty loop moved constants in eleven instantiations that are to stay what they were.  The fence is what this compiler makes
//  of it, not a guarantee: scripts/phase_static.py shows registers and scratch of every phased build after a compiler update.)
#define CTR_MARK(n) if constexpr (!ctr_mark_fence) {} else asm volatile("")
#endif

#ifndef CTR_MIN_WAVES_EU
#define CTR_MIN_WAVES_EU 4
#endif
typedef float float2_ __attribute__((ext_vector_type(2)));
template <int N> struct SiteTag { static constexpr int value = N; };  // which inlined copy of a lambda (CTR_MARK ids)
#define SITE(n) SiteTag<n>()
// d = s * v.{lo|hi} - k.{lo|hi} for both halves of the SGPR pair s: v_pk_fma_f32 with op_sel choosing
// which half of the VGPR pairs v and k is broadcast (vsel/ksel: 0 = low, 1 = high), k negated
// d = s * v.{lo|hi} (both halves of the SGPR pair s times ONE broadcast half of the VGPR pair v)
#define PKMULB(d, s, v, vsel)                                                                                   \
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0," #vsel "] op_sel_hi:[1," #vsel "]" : "=v"(d) : "s"(s), "v"(v))
// d = s * v.{lo|hi} + acc (acc: a full pair)
#define PKFMAB(d, s, v, vsel, acc)                                                                              \
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0," #vsel ",0] op_sel_hi:[1," #vsel ",1]" : "=v"(d) : "s"(s), "v"(v), "v"(acc))
#define PKFMA(d, s, v, vsel, k, ksel)                                                                          \
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0," #vsel "," #ksel "] op_sel_hi:[1," #vsel "," #ksel "] "          \
      "neg_lo:[0,0,1] neg_hi:[0,0,1]"                                                                          \
      : "=v"(d)                                                                                                \
      : "s"(s), "v"(v), "v"(k))
// max over the axes of min(t1, t2) / min over the axes of max(t1, t2); a NaN operand is ignored by
// v_min/v_max (the other operand wins), i.e. that axis' constraint drops out as in the scalar version
__device__ __forceinline__ float slab_lo(float ax, float bx, float ay, float by, float az, float bz) {
  float x, y, z, r;
  asm("v_min_f32 %0, %1, %2" : "=v"(x) : "v"(ax), "v"(bx));
  asm("v_min_f32 %0, %1, %2" : "=v"(y) : "v"(ay), "v"(by));
  asm("v_min_f32 %0, %1, %2" : "=v"(z) : "v"(az), "v"(bz));
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
__device__ __forceinline__ float slab_hi(float ax, float bx, float ay, float by, float az, float bz) {
  float x, y, z, r;
  asm("v_max_f32 %0, %1, %2" : "=v"(x) : "v"(ax), "v"(bx));
  asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(ay), "v"(by));
  asm("v_max_f32 %0, %1, %2" : "=v"(z) : "v"(az), "v"(bz));
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
// the same with one more bound folded in: max(entry distances, mn) / min(exit distances, mx)
__device__ __forceinline__ float slab_lo4(float ax, float bx, float ay, float by, float az, float bz, float mn) {
  float x, y, z, r;
  asm("v_min_f32 %0, %1, %2" : "=v"(x) : "v"(ax), "v"(bx));
  asm("v_min_f32 %0, %1, %2" : "=v"(y) : "v"(ay), "v"(by));
  asm("v_min_f32 %0, %1, %2" : "=v"(z) : "v"(az), "v"(bz));
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(r), "v"(mn));
  return r;
}
__device__ __forceinline__ float slab_hi4(float ax, float bx, float ay, float by, float az, float bz, float mx) {
  float x, y, z, r;
  asm("v_max_f32 %0, %1, %2" : "=v"(x) : "v"(ax), "v"(bx));
  asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(ay), "v"(by));
  asm("v_max_f32 %0, %1, %2" : "=v"(z) : "v"(az), "v"(bz));
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(r), "v"(mx));
  return r;
}
// two adjacent floats of a wave-uniform record as one aligned SGPR pair
__device__ __forceinline__ float2_ ldpair(const CADDR float (&p)[2]) { return *(const CADDR float2_ *)p; }
__device__ __forceinline__ float2_ ldpair2(const CADDR float *p) { return *(const CADDR float2_ *)p; }

// one triangle record as register values (SGPRs: the record is wave-uniform)
struct TriR {
  float2_ ab0, ab1, ab2, pxy;
  float pz;
  uint32_t orig;
  float nx, ny, nz, ke, ke2;
};
__device__ __forceinline__ TriR load_tri(const CADDR DTri &T) {
  TriR r;
  r.ab0 = ldpair(T.ab[0]); r.ab1 = ldpair(T.ab[1]); r.ab2 = ldpair(T.ab[2]);
  r.pxy = ldpair2(&T.px); r.pz = T.pz; r.orig = T.orig;
  r.nx = T.nx; r.ny = T.ny; r.nz = T.nz; r.ke = T.ke; r.ke2 = T.ke2;
  return r;
}

// The same two IEEE results — n = sqrtf(x) and 1.0f / n, correctly rounded — for the whole wave at about half
// the instructions when every active lane's x lies in [2^-80, 2^80].  hipcc's correctly rounded sqrtf / division
// wrap the arithmetic below in denormal scaling (v_div_scale, a pre-multiply by 2^32) and special-case fix-ups
// (v_div_fixup, v_cmp_class) that cannot trigger in that range; what remains is
//   sqrt: s = v_sqrt_f32(x) (1 ulp), then the neighbour whose residual x - s'.s changes sign
//   1/n:  y = v_rcp_f32(n), one Newton step, then two residual corrections q += (1 - n q) y
// in the same operations and order, hence the same bits (checked exhaustively over all 2^24 mantissa / exponent-
// parity patterns by ctr_selftest_exact_math, tests/test_gpu_parity.py).  Any lane outside the range (a zero
// vector, inf, NaN): the whole wave takes the library path.
__device__ __forceinline__ void norm_and_inverse(float x, float &n, float &inv) {
  if (BALLOT(!(x >= 0x1p-80f && x <= 0x1p80f)) != 0ull) {
    CTR_MARK(90);  // library square root and division
    n = sqrtf(x);
    inv = 1.0f / n;
    return;
  }
  CTR_MARK(91);
  const float s0 = __builtin_amdgcn_sqrtf(x);
  const float sm = __uint_as_float(__float_as_uint(s0) - 1u), sp = __uint_as_float(__float_as_uint(s0) + 1u);
  const float rm = __builtin_fmaf(-sm, s0, x), rp = __builtin_fmaf(-sp, s0, x);
  float s = (rm <= 0.0f) ? sm : s0;
  s = (rp > 0.0f) ? sp : s;
  n = s;
  float y = __builtin_amdgcn_rcpf(s);
  const float e = __builtin_fmaf(-s, y, 1.0f);
  y = __builtin_fmaf(e, y, y);
  float q = y;                                   // 1.0f * y
  const float r0 = __builtin_fmaf(-s, q, 1.0f);
  q = __builtin_fmaf(r0, y, q);
  const float r1 = __builtin_fmaf(-s, q, 1.0f);
  inv = __builtin_fmaf(r1, y, q);
}
// a.normalized() and a.norm() together (vector.hpp:77-92), through norm_and_inverse
__device__ __forceinline__ V3 vnormalized_n(V3 a, float &n) {
  float inv;
  norm_and_inverse(a.x * a.x + a.y * a.y + a.z * a.z, n, inv);
  return vscale(a, inv);
}
// The two factors of a light's term (shading.hpp:86-93), each in ONE place: the light set-up tests them for zero before the
// shadow cast ("dark lights") and the continuation shades with them after it, and both must run the same operations.
//   fd = max(0, nn.nd)                          nn: normal.normalized(), nd: the shadow ray's direction
//   fs = pow(max(0, nn.h), phong_exp)           h: the half vector of -incoming->dir.normalized() and nd
// FAST: the half vector's normalisation with the 1-ulp v_rsq_f32 and exp2(e*log2(x)) on the f32 transcendental pipe (relative
// error ~1e-6 wherever the result is not negligible; phong_exp == 0 -> 1); else IEEE sqrt + division and the f64 pow rounded
// once (<= 1 ulp from glibc powf).  Both feed only the colour.
__device__ __forceinline__ float light_fd(V3 nn_, V3 nd) { return smax(0.0f, vdot(nn_, nd)); }
template <bool FAST>
__device__ __forceinline__ float light_fs(V3 nn_, V3 in_dn_, V3 nd, const CADDR DMat &M) {
  const V3 hsum = vadd(vscale(in_dn_, -1.0f), nd);
  const V3 hv = FAST ? vscale(hsum, __builtin_amdgcn_rsqf(vdot(hsum, hsum))) : vnormalized(hsum);
  const float sx = smax(0.0f, vdot(nn_, hv));
  float fs;
  if (FAST) fs = (M.phong_exp == 0.0f) ? 1.0f : __builtin_amdgcn_exp2f(M.phong_exp * __builtin_amdgcn_logf(sx));
  else fs = (float)pow((double)sx, (double)M.phong_exp);
  return fs;
}
// A suspended ray_color activation (shading.hpp:116-154) lives in LDS, never in scratch:
//   hot  fields 0..3 : rgb so far (3), material index | stage << 30 (stage 1 = waiting for the
//                      reflection child, 2 = for the pass-through child; the material record says
//                      how reflective / translucent the surface is)
//   cold fields 4..9 : incoming->start + distance*incoming->dir (3), incoming->dir (3); only
//                      materials that BOTH reflect and transmit need them (A.nf == 10)
// Layout [wave][frame][field][lane]: lane-contiguous dwords, so a push/pop is conflict-free
// whatever each lane's own stack depth is.  bounces_left of a frame is implied by its depth
// (every push decrements it): bl = bounces - depth.
enum { F_R = 0, F_G, F_B, F_MAT, F_PX, F_PY, F_PZ, F_DX, F_DY, F_DZ };  // F_MAT: material index | stage << 30

struct KArgs {
  // hot block, the first 32 bytes: what every cast needs before it reaches a mesh — fetched with ONE s_load_dwordx8 at
  // the head of the trip instead of five dependent scalar loads spread over it (each a round trip the wave waits for)
  const CADDR DPlanePair *planes;
  uint32_t n_plane_recs, n_axis_recs, n_oloop, n_mesh, tlas_root, has_mesh;  // has_mesh: bit 0 = the scene has a mesh, bit 1 = `head` holds the axis triple;
                                                                             // tlas_root: | CTR_TL_HEAD_FLAG when `head` holds that leaf's mesh record
  // cold block, the next 48 bytes: what the continuation needs, fetched together at its start
  const CADDR DObj *objs;      // every object in scene order (hit records)
  const CADDR float *gnorm;
  const CADDR DLight *lights;
  const CADDR DMat *mats;
  uint32_t n_light;
  int bounces;
  uint32_t n_obj, tlas_root2;  // tlas_root2: the top-level tree over the meshes when tlas_root (hot block) names the merged tree
  const CADDR DObj *oloop;     // spheres and stand-alone triangles (sequential loop)
  const CADDR DObj *meshes;    // meshes with >= 1 triangle, in top-level-BVH leaf order
  uint32_t tlas_begin;
  float tl_mn[3], tl_mx[3];    // box of all meshes (margin of the top-level walk)
  const CADDR DTri *tris;
  const CADDR DNode *nodes;    // top-level tree over the meshes (two-wide nodes)
  const CADDR DNode4 *nodes4;  // per-mesh trees (four-wide nodes)
  const CADDR DCam *cams;      // one camera per frame of the batch (all w x h)
  uint32_t w, h;
  uint32_t first_frame, n_frames;
  uint64_t frame_stride_px;    // pixels between consecutive frames in the output buffers
  DRows rows;
  float fudge;
  uint32_t nf;        // LDS dwords per stack frame: 4, or 10 when some material reflects AND transmits
  uint32_t frames;    // LDS stack frames per lane: the recursion depth that can be reached (bounces, or 1 when no
                      // material reflects or transmits: ray_color then never recurses)
  const CADDR uint32_t *order;  // dispatch slot -> wave (tile) index, or null = identity
  uint32_t *cost;               // per wave (tile): shader-clock ticks it took, or null
  // "Host delivery" (below): null group_done = the outputs are written in place
  float *host_depth, *host_color, *host_normal;
  uint32_t *group_done;
  float *uv_out;      // KV_UV: texture coordinates of the primary hit, 2 floats per pixel
  uint32_t ss_log2;   // KV_SS: log2 of the samples per axis (1, 2 or 3); w, h and rows are those of the s*w x s*h sample frame
  // "Lens render" (KV_RAYS): the primary rays, 3 floats per pixel (sample) of the whole w x h frame, row-major by GLOBAL row,
  // and phong's ambient factor (the plain render takes the camera's).  They fill the gap in front of the 64-byte aligned
  // scene head, so nothing else in the argument block moves.
  const float *ray_origin, *ray_dir;
  float ray_ambient;
  // "Scene head" (scene_device.h DSceneHead): the first plane triple and the first mesh record INSIDE the argument block.
  // Their address is kernarg base + constant, so the planes are requested in the same burst as the hot block (one
  // scalar round trip at the head of a cast, not two dependent ones) and the mesh record without fetching `meshes`
  // first.  Only scalar loads read it, like the rest of the kernarg segment.
  DSceneHead head;
};

static_assert(offsetof(KArgs, planes) == 0 && offsetof(KArgs, has_mesh) == 28, "KArgs: the hot block is the first eight dwords");
static_assert(offsetof(KArgs, objs) == 32 && offsetof(KArgs, mats) == 56 && offsetof(KArgs, bounces) == 68, "KArgs: the cold block follows");

// The kernel's whole argument block as it lies in the kernarg segment: the output pointers are read from there where a
// pixel is written (the first cast's depth and normal, the colour when the pixel is finished) instead of living in
// eight SGPRs across every cast — where the compiler parked them in VGPR lanes and fetched them back after each cast's
// mesh walk (eight v_readlane per cast for pointers two casts in thirty use).
struct KParams {
  KArgs A;
  float *depth_out, *color_out, *normal_out;
  unsigned long long *counters;
};
static_assert(offsetof(KArgs, ss_log2) == 288 && offsetof(KArgs, ray_origin) == 296 && offsetof(KArgs, head) == 320, "KArgs: the lens arguments lie in the padding behind ss_log2");
static_assert(sizeof(KArgs) % 64 == 0 && offsetof(KArgs, head) % 64 == 0 && offsetof(KParams, depth_out) == sizeof(KArgs), "KParams mirrors the kernel's parameter list; the scene head lies on 64-byte lines");

// ---- Host delivery ----
// ctr_render hands the kernel page-locked HOST buffers.  Storing the pixels there tile by tile works (the memory is
// device-visible) but reaches PCIe as 32- and 96-byte runs: 43 GB/s for the stores alone, where one DMA of the frame
// makes 56 (scripts/pcie_store.hip).  So the tiles go to a tile-major staging area in device memory, and the wave
// that completes a GROUP of 64/TW horizontally adjacent tiles (64 x TH pixels; a counter per group) copies the
// group into the host buffers in runs of 256 / 768 bytes — the DMA's rate, but spread over the whole launch instead
// of after it.  The order the tiles are dispatched in keeps the tiles of a group together (tile_order.hip order_block).

// What a lane casts its next ray for, and how deep its recursion stack is, share ONE register (a VGPR less to carry
// through the cast loops): low 16 bits = stack depth; bit 31 = a shadow-loop cast, bit 30 = the pixel is finished,
// neither = a radiance cast.  Every test is a single compare.
constexpr uint32_t MSP_SHADOW = 0x80000000u, MSP_DONE = 0x40000000u;
// Room-safe lanes (any-hit builds; DSceneHead::room_*, DESIGN.md "Shadow casts from inside a plane room"): bit 29 says that the
// hit point the lane's shadow rays start from passed the lane predicate of the launch's room facts — set once per shaded hit,
// kept through `msp |= MSP_SHADOW` from light to light, gone wherever msp is rebuilt for the next radiance cast (stack depth
// or MSP_DONE alone).  Below bit 30, so every test here stays the single compare it was.
constexpr uint32_t MSP_ROOM = 0x20000000u;
// Dark lights (the DARK builds; CTR_HEAD_DARK of the scene head, DESIGN.md "Dark lights"): bit 28 says that the light the lane's shadow ray
// goes to cannot change the lane's pixel — set or cleared where the ray is made, so it lasts for that one light; it survives
// `| MSP_SHADOW` and is gone, like MSP_ROOM, wherever msp is rebuilt.
constexpr uint32_t MSP_DARK = 0x10000000u;
#define MSP_ACTIVE(m) ((int)(m) < 0x40000000)          /* radiance or shadow */
#define MSP_IS_SHADOW(m) ((int)(m) < 0)
#define MSP_IS_RADIANCE(m) ((uint32_t)(m) < 0x40000000u)
#define MSP_DEPTH(m) ((int)((m) & 0xFFFFu))
enum { ACT_NONE = 0, ACT_LIGHT = 1, ACT_BOUNCE = 2, ACT_UNWIND = 3 };

// (launch bounds: the 6-wave builds, and every phased build — the opaque parents of the builds without KV_OCC6 run at 6 waves
//  per SIMD as well, by the compiler's choice at 75 ... 79 VGPRs; with two inlined trips and no bound it chose 83 ... 87 for
//  their twins, five waves.  The bound keeps a phased build in its parent's class; profiles/r09/phase_static.txt.)
template <uint32_t KV, uint32_t SHAPE = KS_GENERAL, bool ROOM = false, uint32_t OPQ = KO_PARENT, bool DARK = false, bool PHASED = false>
__global__ __launch_bounds__(WG_THREADS, ((KV & KV_OCC6) || PHASED) ? 6 : CTR_MIN_WAVES_EU) void render_kernel(KArgs A, float *__restrict__ depth_out,
                                                            float *__restrict__ color_out,
                                                            float *__restrict__ normal_out,
                                                            unsigned long long *__restrict__ counters) {
  constexpr bool PREFILTER = (KV & KV_PREFILTER) != 0;
  constexpr bool ANYHIT = (KV & KV_ANYHIT) != 0;
  constexpr bool COUNT = (KV & KV_COUNT) != 0;
  constexpr bool BVH = (KV & KV_BVH) != 0;
#ifdef CTR_WAVELOG
  constexpr bool STATS = true;
#else
  constexpr bool STATS = (KV & KV_STATS) != 0;
#endif
  constexpr bool FASTPOW = (KV & KV_FASTPOW) != 0;
  constexpr bool HOSTOUT = (KV & KV_HOSTOUT) != 0;  // "Host delivery"
  constexpr bool UV = (KV & KV_UV) != 0;            // ray_cast's tex_coords of the primary cast as a fourth output
  // "Supersampling": the launch renders the s*w x s*h sample frame (s = 1 << ss_log2 divides TW and TH, so an s x s block
  // of samples lies inside one wave); depth and normal of a pixel are those of its sample (0, 0), its colour the mean of
  // the block, reduced across the lanes at the end of the wave (include/cutrace_aa.h has the definition and the order)
  constexpr bool SS = (KV & KV_SS) != 0;
  static_assert(!SS || !((KV & (KV_HOSTOUT | KV_STATS | KV_UV)) != 0), "the supersampled frame leaves through device buffers, three outputs");
  // ray_cast's ninth argument (ray_cast.hpp:30,39-40: `if (ignore_transparent && is_transparent(mat)) continue;`).  Every caller
  // of the reference passes false; with IGNTR the cast of kernel.hpp:52 — the one depth, normal and tex_coords come from — is
  // made with true, as a trip of its own before ray_color's first cast (shading.hpp:123, false), which it otherwise shares
  constexpr bool IGNTR = (KV & KV_IGNTR) != 0;
  constexpr bool MERGE = (KV & KV_MERGE) != 0;      // "merged walk": the top-level item may be the pseudo mesh over all meshes' triangles
  static_assert(!MERGE || BVH, "the merged tree is a BVH walk");
  // "Lens render": the primary ray of a pixel (sample) is the caller's (origin, direction) instead of cam::get_ray's; a ray
  // with a non-finite origin, or whose normalised direction is not finite or is (0, 0, 0), is MASKED: no cast, the miss values
  // (include/cutrace_lens.h has the definition).  Only the prologue differs: origin and direction are per-lane VGPRs in the
  // cast loops anyway.
  constexpr bool RAYS = (KV & KV_RAYS) != 0;
  static_assert(!RAYS || !((KV & (KV_HOSTOUT | KV_STATS | KV_UV | KV_COUNT | KV_IGNTR | KV_MERGE)) != 0), "the lens render leaves through device buffers, three outputs, two-level walk");
  // "Launch shape" (kernel_choice.h launch_shape): the scene has no sphere and no stand-alone triangle, and exactly one mesh,
  // whose record is DSceneHead::mesh.  The object loop then runs zero times and the top-level walk consists of that one leaf:
  // both are compiled out — their loop skeletons, the stack of the walk and the leaf's bookkeeping are scalar instructions every
  // trip pays for, and the kernel runs at its instruction-issue limit.  Nothing a taken path computes changes.
  constexpr bool ONE_MESH = SHAPE == KS_ONE_MESH;
  static_assert(SHAPE == KS_GENERAL || SHAPE == KS_ONE_MESH, "launch shapes: kernel_choice.h");
  // "Room-safe lanes" (MSP_ROOM above; DESIGN.md "Shadow casts from inside a plane room"): the code that lets a shadow trip skip its
  // plane tests exists only in the instantiations launched for it — ROOM: a one-mesh launch whose scene head carries room facts
  // (ctr_launch_render picks <KV, KS_ONE_MESH, true> then) — and in the any-hit statistics builds, which count the trips.  Every
  // other instantiation is, instruction for instruction, what it was without it: a launch that cannot skip pays nothing.
  static_assert(!ROOM || ONE_MESH, "room-safe lanes: the one-mesh builds");
  constexpr bool ROOM_CODE = ANYHIT && (ROOM || STATS);
  static_assert(!ONE_MESH || (KV & ~(KV_OCC6 | KV_HOSTOUT)) == (KV_PREFILTER | KV_BVH | KV_ANYHIT | KV_FASTPOW), "KS_ONE_MESH: the builds of CTR_SHAPE_KERNELS");
  // "Opaque build" (kernel_choice.h KO_*; DESIGN.md "The opaque one-mesh build"): an any-hit build is launched only when every
  // material's transparency is exactly zero, so ray_color never casts a pass-through child: `do_trans` is false in every lane.
  // OPAQUE compiles that half of the continuation out — the transparency read and its f64 compare, the six-dword push, the
  // unwind's pass-through stage — and with it the reasons to keep the incoming direction and a second copy of the hit point
  // alive across the hit's shadow trips: the radiance ray's direction is `rd` where the hit record needs it, and in the
  // one-mesh shape (plane or mesh hits only) the hit point is `ro` from the hit record to the bounce.  Nothing a taken path
  // computes changes.
  constexpr bool OPAQUE = OPQ != KO_PARENT;
  static_assert(OPQ == KO_PARENT || OPQ == KO_OPAQUE, "opaque builds: kernel_choice.h");
  static_assert(!OPAQUE || (ANYHIT && ONE_MESH), "the opaque builds are any-hit one-mesh builds");
  // "Dark lights" (MSP_DARK above; DESIGN.md "Dark lights"): in an any-hit build a shadow cast only decides whether the light's
  // term  fd*ld + fs*ls  is added to `fin` or not.  Where fd and fs are both zero, every colour of the scene is finite and
  // bounded (CTR_HEAD_DARK of the scene head) and no channel of `fin` is -0, adding the term — a signed zero per channel — leaves
  // `fin` bit for bit, so the cast cannot be observed: the lane sits the trip out (it is still counted as a cast), and a trip whose
  // lanes all do goes straight to the continuation.  The code exists only in the instantiations launched for it — DARK: an opaque
  // build whose scene head carries the fact (ctr_launch_render picks <KV, KS_ONE_MESH, ROOM, KO_OPAQUE, true> then) — and, counting
  // only, no lane retired, in the any-hit statistics builds, which read the fact from the head.  Every other instantiation is,
  // instruction for instruction, what it was without it: a launch without the fact pays nothing.
  static_assert(!DARK || OPAQUE, "dark lights: the opaque builds");
  constexpr bool DARK_CODE = DARK || (ANYHIT && STATS);
  // "Phased builds" (kernel_choice.h phased_build; DESIGN.md "Phased opaque builds"): in an opaque build every active lane runs
  // the same sequence — a radiance trip, n_light shadow trips (an any-hit shadow loop ends with its first trip; a dark lane sits
  // its trip out but takes it), a radiance trip one frame deeper — and leaves it only by ending (MSP_DONE).  So what a trip is
  // cast for, and towards which light, is the same in every active lane: the wave-uniform `phase` below, 0 = a radiance trip,
  // k = the shadow trip towards light k - 1.  PHASED compiles the trip body twice, once per kind (TRIP_RADIANCE / TRIP_SHADOW),
  // behind one scalar branch; in a copy the kind, the light index and everything derived from them are constants or scalars,
  // the mode bits of `msp` and the per-lane `li` are not kept, and the continuation holds that kind's branch alone.  The
  // arithmetic of every taken path is the generic body's (TRIP_ANY), in the same order.  Every other instantiation is,
  // instruction for instruction, what it was without it.
  static_assert(!PHASED || OPAQUE, "phased builds: the opaque builds");
  enum { TRIP_ANY = 0, TRIP_RADIANCE = 1, TRIP_SHADOW = 2 };
  // wave-level work counters (STATS build only): [0] casts, [1] BVH nodes visited, [2] triangle
  // prefilters, [3] exact tests, [4] mesh entries (AABB ballot != 0), [5] sum of active lanes per cast,
  // and how many of the 64 lanes had a use for the wave-level work: [6] lanes whose ray meets one of the
  // visited node's child boxes, [7] lanes inside the leaf's box at a prefilter, [8] lanes in an exact test
  // and what a walk by every lane for itself would take, counted in steps of the whole wave: per mesh entry the LARGEST
  // number of [9] node visits and [10] triangle tests any one lane has a use for (the bound on what a per-lane walk
  // below some depth could save: DESIGN.md "Per-lane walk")
  unsigned long long st[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#ifdef CTR_TIMING
  // diagnostic build only: shader-clock stamps per wave -> shards[4..13] = {cast setup, planes, object
  // loop, top-level walk + mesh AABB, mesh entry setup, BVH walk without leaves, leaves, radiance
  // continuation, rest of the continuation, whole wave}
  unsigned long long tm[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long tm_start = __builtin_readcyclecounter();
#define TSTAMP(v) const unsigned long long v = __builtin_readcyclecounter()
#define TACC(i, a, b) tm[i] += (b) - (a)
#else
#define TSTAMP(v)
#define TACC(i, a, b)
#endif

#ifdef CTR_WAVELOG
  const unsigned long long wl_start = __builtin_amdgcn_s_memrealtime();  // 100 MHz
#endif
  CTR_MARK(0);  // wave prologue
  const uint32_t w = A.w, h = A.h;
  const uint32_t lane = threadIdx.x & 63u;
  // wave-uniform by construction; with one wave per workgroup (the shipped build) a compile-time zero, so that no LDS base
  // offset derived from it has to be carried (parked in a VGPR lane and fetched back every cast) through the kernel
  const uint32_t wave_in_wg = WAVES_PER_WG == 1 ? 0u : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t slot = (blockIdx.x * WAVES_PER_WG) + wave_in_wg;
  const uint32_t tiles_x = (w + TW - 1) / TW;
  const uint32_t tiles_y = (A.rows.n_rows + TH - 1) / TH;
  const uint32_t tiles_frame = tiles_x * tiles_y;
  if (slot >= tiles_frame * A.n_frames) return;  // whole wave exits together
  // Dispatch order.  Waves differ 10x in cost and the hardware hands them out in blockIdx order, so
  // with tiles in image order the last quarter of a frame is a tail of a few slow waves on an
  // otherwise empty GPU.  Every launch records what each tile cost; the next launch of the same
  // shape starts the expensive tiles first (longest-processing-time-first list scheduling).
  const unsigned long long t_wave0 = __builtin_readcyclecounter();
  const uint32_t wave = A.order ? A.order[slot] : slot;
  if (wave >= tiles_frame * A.n_frames) return;  // cannot happen with a valid order; never write out of bounds
  // batch of frames (a camera path): frame-major waves, one camera per frame (wave-uniform)
  const uint32_t frame = wave / tiles_frame;
  const uint32_t tile = wave - frame * tiles_frame;
  const CADDR DCam &cam = A.cams[A.first_frame + frame];
  const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
  const uint32_t x_id = tx * TW + (lane % TW);
  const uint32_t k_row = ty * TH + (lane / TW);  // local (compact) row
  // local row -> global image row (interleaved row blocks, see ctr_rows).  In a batch the part a
  // rank renders may rotate from frame to frame (part_stride), which balances ranks whose row
  // blocks differ in cost.
  uint32_t y_id;
  if (A.rows.n_parts <= 1) y_id = A.rows.row_begin + k_row;
  else {
    const uint32_t part_f = (A.rows.part + frame * A.rows.part_stride) % A.rows.n_parts;
    const uint32_t b0 = A.rows.row_begin / A.rows.block_rows;
    const uint32_t first = b0 + ((part_f + A.rows.n_parts - (b0 % A.rows.n_parts)) % A.rows.n_parts);
    const uint32_t j = k_row / A.rows.block_rows;
    y_id = (first + j * A.rows.n_parts) * A.rows.block_rows + (k_row % A.rows.block_rows);
  }
  const bool in_image = x_id < w && k_row < A.rows.n_rows && y_id < A.rows.row_end;
  // kernel.hpp:54 (compact buffer).  Recomputed from the lane id at its three uses rather than kept
  // in two VGPRs for the whole wave: registers, not instructions, are what this kernel is short of.
  // (SS: the tile's first OUTPUT pixel, in the w/s-wide frame)
  const uint32_t tile_px0 = SS ? ((ty * TH) >> A.ss_log2) * (w >> A.ss_log2) + ((tx * TW) >> A.ss_log2) : ty * TH * w + tx * TW;  // wave-uniform
  // a pixel's three floats: in place, or — staged — written THROUGH to memory (agent scope), because the wave that
  // copies the group to the host usually runs on another XCD, whose L2 is not coherent with this one
  auto store3 = [&](float *__restrict__ out, size_t px_id, V3 v) {
    if (HOSTOUT) {
      __hip_atomic_store(out + 3 * px_id + 0, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(out + 3 * px_id + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(out + 3 * px_id + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      out[3 * px_id + 0] = v.x;
      out[3 * px_id + 1] = v.y;
      out[3 * px_id + 2] = v.z;
    }
  };
  // the lane's number from the hardware (two v_mbcnt) wherever a per-lane address is formed inside the loop: neither the
  // lane id nor an address derived from it is then carried through the cast loops in a register
  auto lane_now = [&]() -> uint32_t { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); };
  auto px_index = [&]() -> size_t {
    const uint32_t l = lane_now();  // recomputed here: hoisted out of the loop the addresses would be spilled to scratch
    if (HOSTOUT) return (size_t)wave * 64u + l;  // tile-major staging ("Host delivery")
    if constexpr (SS) {  // the output pixel the lane's sample belongs to: (k_row / s) * (w / s) + x_id / s
      const uint32_t ls = ((const CADDR KArgs *)__builtin_amdgcn_kernarg_segment_ptr())->ss_log2;
      if constexpr (RAYS) return (size_t)(tile_px0 + ((l / TW) >> ls) * (w >> ls) + ((l % TW) >> ls));  // (one frame: launch)
      return (size_t)frame * A.frame_stride_px + (size_t)(tile_px0 + ((l / TW) >> ls) * (w >> ls) + ((l % TW) >> ls));
    }
    // (RAYS: one frame, launch checks; the frame offset, computed before the loop for a masked pixel, would be kept for the
    //  stores inside it — in scratch, in the 6-wave build)
    if constexpr (RAYS) return (size_t)(tile_px0 + (l / TW) * w + (l % TW));
    return (size_t)frame * A.frame_stride_px + (size_t)(tile_px0 + (l / TW) * w + (l % TW));
  };

  // SS: the lane that holds sample (0, 0) of its block — x_id % s == 0 && k_row % s == 0 — is the one that stores the pixel
  auto ss_kept = [&]() -> bool {
    const uint32_t l = lane_now();
    const uint32_t m = (1u << ((const CADDR KArgs *)__builtin_amdgcn_kernarg_segment_ptr())->ss_log2) - 1u;
    return (((l % TW) | (l / TW)) & m) == 0u;
  };

  // ---- cam::get_ray, default_schema.hpp:376-386 ----
  V3 ro, rd;
  bool masked = false;  // RAYS: an in-image lane without a ray
  if constexpr (RAYS) {
    const CADDR KArgs *AR = (const CADDR KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const float *const po = AR->ray_origin, *const pd = AR->ray_dir;
    ro = mk(0.f, 0.f, 0.f);
    rd = mk(0.f, 0.f, 1.f);
    if (in_image) {  // (in_image: x_id < w and y_id < h, so the index is inside the caller's w*h rays)
      const size_t i = ((size_t)y_id * (size_t)w + (size_t)x_id) * 3u;
      ro = mk(po[i + 0], po[i + 1], po[i + 2]);
      rd = mk(pd[i + 0], pd[i + 1], pd[i + 2]);
    }
    rd = vnormalized(rd);
    const bool o_fin = __builtin_isfinite(ro.x) && __builtin_isfinite(ro.y) && __builtin_isfinite(ro.z);
    const bool d_fin = __builtin_isfinite(rd.x) && __builtin_isfinite(rd.y) && __builtin_isfinite(rd.z);
    const bool d_zero = rd.x == 0.f && rd.y == 0.f && rd.z == 0.f;
    masked = in_image && !(o_fin && d_fin && !d_zero);
  } else {
    const float fw = (float)w, fh = (float)h;
    const float aspect = fw / fh;
    const V3 right = mk(cam.right[0], cam.right[1], cam.right[2]);
    const V3 up = mk(cam.up[0], cam.up[1], cam.up[2]);
    const V3 fwd = mk(cam.forward[0], cam.forward[1], cam.forward[2]);
    V3 x_v = vscale(right, (((float)x_id / fw) - 0.5f) * aspect);
    V3 y_v = vscale(up, 0.5f - ((float)y_id / fh));
    ro = mk(cam.pos[0], cam.pos[1], cam.pos[2]);
    rd = vnormalized(vadd(vadd(x_v, y_v), fwd));
  }
  const float ambient = RAYS ? 0.f : cam.ambient;  // (RAYS: the launch's, read where phong starts)

  // ---- per-lane state machine ----
  uint32_t msp = (in_image && !masked) ? 0u : MSP_DONE;  // mode | stack depth (MSP_*); bounces left for the current activation = bounces - depth
  bool first_trip = true;   // wave-uniform: every in-image lane shades its primary hit in the first trip
  uint32_t wave_dbits = 0u; // wave-uniform: max finite depth bits of the tile (kernel.hpp:120-125)
  float min_t = A.fudge;
  extern __shared__ float lds_stack[];
#define STK(frame, field) (lds_stack + (size_t)wave_in_wg * A.frames * A.nf * 64 + lane_now())[((frame) * A.nf + (field)) * 64]
  V3 in_d = rd;             // direction of the radiance ray being shaded ("incoming"); its start is `ro` until the hit
  V3 nn = mk(0, 0, 0), pos = mk(0, 0, 0);  // (the hit point itself lives in `ro` from the hit on: it is
                                           //  the origin of every shadow ray of that hit)
  V3 in_dn = mk(0, 0, 0);   // incoming->dir.normalized() (shading.hpp:90,131; default_schema.hpp:245)
  // PARK (the 6-waves-per-SIMD build): five dwords of shading state that no cast reads — in_dn and two components of
  // nn, written once per shaded hit, read once per light — live in LDS behind the wave's stack instead of in VGPRs.
  // They are what the register allocator spilled to scratch at 80 VGPRs (write-back traffic all frame long: 1.9x the
  // compulsory bytes on the bunny frame, 3.5x with 64 000 triangles); five, because LDS is handed out in 1280-byte
  // granules and 5 KB of stack (bounces 5) + 1280 B is the most that still lets 24 waves share a CU
  // (profiles/r03/lds_granule.txt).
  constexpr bool PARK = (KV & KV_OCC6) != 0;
#define PRK(i) (lds_stack + (size_t)WAVES_PER_WG * A.frames * A.nf * 64 + (size_t)wave_in_wg * 5 * 64 + lane_now())[(i) * 64]
  auto set_in_dn = [&](V3 v) { if (PARK) { PRK(0) = v.x; PRK(1) = v.y; PRK(2) = v.z; } else in_dn = v; };
  auto get_in_dn = [&]() -> V3 { return PARK ? mk(PRK(0), PRK(1), PRK(2)) : in_dn; };
  auto set_nn = [&](V3 v) { if (PARK) { PRK(3) = v.x; PRK(4) = v.y; nn.z = v.z; } else nn = v; };
  auto get_nn = [&]() -> V3 { return PARK ? mk(PRK(3), PRK(4), nn.z) : nn; };
  V3 fin = mk(0, 0, 0);     // phong accumulator ("final")
  float light_dist = 0.f, intensity = 0.f;
  uint32_t mat_i = 0, li = 0;
  V3 out_rgb = mk(0, 0, 0);
  bool recv_mesh = false;   // STATS only: the surface this lane's shadow rays start on is a mesh / triangle
  // casts of the whole wave, counted on the scalar unit; the duplicated primary cast (kernel.hpp:52) counts too
  // (IGNTR: the kernel.hpp:52 cast is a trip of its own and is counted there)
  unsigned long long n_casts = IGNTR ? 0ull : (unsigned long long)__builtin_popcountll(BALLOT(in_image && !masked));
  unsigned long long n_aabb_tris = 0;

  // Cold kernel arguments — what only the continuation needs (hit records, lights, materials) — are read from
  // the kernarg segment where they are used instead of living in SGPRs across the object / BVH / triangle loops:
  // the loops need every scalar register, and an argument kept through them is spilled to a VGPR lane and comes
  // back by v_readlane (a half-rate VALU instruction per dword, every trip); an s_load from the scalar cache costs
  // no VALU slot.  The pointer is made opaque once per trip so that the loads stay inside the trip.
  const CADDR KArgs *AK = (const CADDR KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  if constexpr (RAYS) {
    // a masked pixel is finished before the first cast: kernel.hpp:55-56's miss values, colour (0, 0, 0); it is not counted
    // and, its depth being infinite, does not enter max_depth.  SS: depth and normal from the lane that holds sample (0, 0);
    // the colour is parked as zeros in the lane's frame 0, where the reduction after the loop finds it
    if (masked) {
      const V3 zero = mk(0.f, 0.f, 0.f);
      if constexpr (SS) {
        if (ss_kept()) {
          const size_t px_id = px_index();
          ((const CADDR KParams *)AK)->depth_out[px_id] = INFINITY;
          store3(((const CADDR KParams *)AK)->normal_out, px_id, zero);
        }
        STK(0, F_R) = 0.f; STK(0, F_G) = 0.f; STK(0, F_B) = 0.f;
        msp = MSP_DONE | 1u;
      } else {
        const size_t px_id = px_index();
        ((const CADDR KParams *)AK)->depth_out[px_id] = INFINITY;
        store3(((const CADDR KParams *)AK)->normal_out, px_id, zero);
        store3(((const CADDR KParams *)AK)->color_out, px_id, zero);
      }
    }
  }
  uint32_t phase = 0u;        // PHASED, wave-uniform: the kind of the trip (0 radiance, k = the shadow trip towards light k - 1)
  uint32_t phase_lights = 0u; // PHASED, wave-uniform: n_light as the trip's continuation read it
  while (BALLOT(MSP_ACTIVE(msp)) != 0ull) {
    // one trip: render_trip.h, included as text — once, or in a phased build once per kind behind the build's one scalar branch
    if constexpr (PHASED) {
      if (phase == 0u) {
#define CTR_TRIP_KIND TRIP_RADIANCE
#include "render_trip.h"
#undef CTR_TRIP_KIND
      } else {
#define CTR_TRIP_KIND TRIP_SHADOW
#include "render_trip.h"
#undef CTR_TRIP_KIND
      }
      // the next trip's kind: after the radiance trip the lights in turn, after the last light — or with no light at all — a
      // radiance trip again
      phase = phase == phase_lights ? 0u : phase + 1u;
    } else {
#define CTR_TRIP_KIND TRIP_ANY
#include "render_trip.h"
#undef CTR_TRIP_KIND
    }
  }
  if constexpr (SS) {
    // ---- "Supersampling": the mean of each s x s block of parked sample colours, in float32 and in a fixed order ----
    // along x by repeated halving (a[i] = a[2i] + a[2i+1]), then along y in the same way, then times 1 / (s*s).  A sum of
    // two floats does not depend on the operands' order, so the xor butterfly gives every lane of a block the tree's value.
    // The lanes of a block are inside or outside the image together (w, h and the rows are multiples of s); what lanes
    // outside it read from their never-written frame is added only among themselves and never stored.
    const uint32_t ls = AK->ss_log2;
    V3 c = mk(STK(0, F_R), STK(0, F_G), STK(0, F_B));
    for (uint32_t k = 0; k < ls; k++) {
      const int off = 1 << k;
      c = mk(c.x + __shfl_xor(c.x, off), c.y + __shfl_xor(c.y, off), c.z + __shfl_xor(c.z, off));
    }
    for (uint32_t k = 0; k < ls; k++) {
      const int off = TW << k;
      c = mk(c.x + __shfl_xor(c.x, off), c.y + __shfl_xor(c.y, off), c.z + __shfl_xor(c.z, off));
    }
    const float inv = 1.0f / (float)(1u << (2u * ls));
    if (msp == (MSP_DONE | 1u) && ss_kept()) store3(((const CADDR KParams *)AK)->color_out, px_index(), vscale(c, inv));
  }
#undef STK
#undef PRK

  CTR_MARK(56);  // wave epilogue
  // (the tile's cost for the next launch's order ends here: what the group copy below costs the one wave that makes
  //  it depends on the link, not on the tile)
  const unsigned long long t_wave1 = HOSTOUT ? __builtin_readcyclecounter() : 0ull;
  if (HOSTOUT) {
    const CADDR KArgs *AE = (const CADDR KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(AE));  // the kernel arguments once more (see AK): none of this is worth an SGPR across the loop
    // "Host delivery": this tile is complete; the wave that completes its group copies the group to the host
    const uint32_t e_w = AE->w, e_tiles_x = (e_w + TW - 1) / TW, e_ty = wave / e_tiles_x, e_tx = wave - e_ty * e_tiles_x;
    const uint32_t groups_x = (e_tiles_x + GROUP_TILES - 1) / GROUP_TILES;
    const uint32_t gx = e_tx / GROUP_TILES, t0 = gx * GROUP_TILES;
    const uint32_t nt = e_tiles_x - t0 < GROUP_TILES ? e_tiles_x - t0 : GROUP_TILES;
    uint32_t *const done = AE->group_done + (e_ty * groups_x + gx);
    // The tile's pixels were written through (store3) and have arrived when the counter is incremented: an agent-
    // scope release fence here would write this XCD's whole L2 back, and the acquire below invalidate it, once per
    // wave — 3 ms per frame, measured.  The copy reads with agent-scope loads, which do not hit a stale L2 line.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0;
    if (lane == 0) old = atomicAdd(done, 1u);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old == nt - 1) {
      CTR_MARK(57);  // host delivery: copy a group
      // (the counter keeps its final value nt: ctr_render.cpp clears the counters before every launch and, after it, checks
      //  that every group counted all its tiles — a launch cut short cannot leave a later one a poisoned counter, and a
      //  group that was never delivered is an error, not stale pixels)
      const uint32_t row0 = e_ty * TH, n_rows = AE->rows.n_rows;
      const uint32_t rows_valid = n_rows - row0 < (uint32_t)TH ? n_rows - row0 : (uint32_t)TH;
      const uint32_t x0 = t0 * TW;
      const uint32_t cols = e_w - x0 < nt * TW ? e_w - x0 : nt * TW;  // pixels of the group inside the image
      const size_t stile0 = (size_t)(e_ty * e_tiles_x + t0) * 64u;   // the group's first staging pixel
      float *const h_depth = AE->host_depth, *const h_color = AE->host_color, *const h_normal = AE->host_normal;
      // four rows at a time: 28 loads in flight, then their 28 stores (an atomic load is not moved across a
      // store by the compiler, and a copy that waits for every load in turn would take ~100 us per group)
      constexpr uint32_t RB = TH < 4 ? TH : 4;
      for (uint32_t rb = 0; rb < rows_valid; rb += RB) {
        float vd[RB], vc[RB][3], vn[RB][3];
#pragma unroll
        for (uint32_t q = 0; q < RB; q++) {
          const uint32_t r = rb + q;
          const bool row_ok = r < rows_valid;
          vd[q] = 0.f;
          if (row_ok && lane < cols)
            vd[q] = __hip_atomic_load(depth_out + stile0 + (size_t)(lane / TW) * 64u + r * TW + lane % TW, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (uint32_t j = 0; j < 3; j++) {
            const uint32_t f = j * 64u + lane, p = f / 3u;  // float f of the row's 3*cols, pixel p of the row
            vc[q][j] = vn[q][j] = 0.f;
            if (row_ok && p < cols) {
              const size_t src = (stile0 + (size_t)(p / TW) * 64u + r * TW + p % TW) * 3u + f % 3u;
              vc[q][j] = __hip_atomic_load(color_out + src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              vn[q][j] = __hip_atomic_load(normal_out + src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
#pragma unroll
        for (uint32_t q = 0; q < RB; q++) {
          const uint32_t r = rb + q;
          if (r >= rows_valid) break;
          const size_t dst_px = (size_t)(row0 + r) * e_w + x0;
          // written through to the host (system scope): 2-7 % faster per call than plain stores, which leave it to the
          // L2 when the lines go out (the host buffers may be cached there like any other memory)
          if (lane < cols) __hip_atomic_store(h_depth + dst_px + lane, vd[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
          for (uint32_t j = 0; j < 3; j++) {
            const uint32_t f = j * 64u + lane;
            if (f / 3u < cols) {
              __hip_atomic_store(h_color + dst_px * 3u + f, vc[q][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              __hip_atomic_store(h_normal + dst_px * 3u + f, vn[q][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
        }
      }
    }
  }

  CTR_MARK(58);
  if (A.cost && lane == 0) {
    const unsigned long long dt = ((HOSTOUT ? t_wave1 : __builtin_readcyclecounter()) - t_wave0) >> 6;
    const uint32_t c = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt;
    A.cost[wave] = c;
  }
#ifdef CTR_WAVELOG
  // diagnostic build only: lane 0 overwrites its pixel's normal with {start, end} of the wave (10 ns ticks)
  if (lane == 0 && in_image) {
    const size_t px_id = px_index();
    const unsigned long long wl_end = __builtin_amdgcn_s_memrealtime();
    normal_out[px_id * 3 + 0] = __uint_as_float((uint32_t)wl_start);
    normal_out[px_id * 3 + 1] = __uint_as_float((uint32_t)wl_end);
    normal_out[px_id * 3 + 2] = __uint_as_float((uint32_t)(st[1] | (st[2] << 12) | (st[3] << 24)));  // nodes, prefilters, exact
  }
#endif
  // ---- per-wave reductions -> 2-3 atomics per wave, spread over CTR_SHARDS cache lines ----
  // (all waves adding into ONE address serialise at the memory side: 0.76 ms per 1080p frame,
  //  measured; one 128-byte shard per wave%CTR_SHARDS costs nothing measurable.  tile_order.hip after_render
  //  then adds the shards into the caller's counters and clears them.)
  if (counters) {
    const unsigned long long c = n_casts;
    const uint32_t dbits = wave_dbits;
    unsigned long long t = n_aabb_tris;
    if (COUNT) {
      for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    }
    unsigned long long *sh = counters + (size_t)(wave % CTR_SHARDS) * CTR_SHARD_WORDS;
    if (STATS && lane == 0) {
      for (int q = 0; q < 11; q++) atomicAdd(&sh[4 + q], st[q]);
    }
#ifdef CTR_TIMING
    if (lane == 0) {
      tm[9] = __builtin_readcyclecounter() - tm_start;
      for (int q = 0; q < 10; q++) atomicAdd(&sh[4 + q], tm[q]);
    }
#endif
    if (lane == 0) {
      atomicAdd(&sh[0], c);
      atomicMax(&sh[1], (unsigned long long)dbits);
      if (COUNT) atomicAdd(&sh[2], t);
    }
  }
}
#undef CTR_MARK

// One launch of `kernel` = render_kernel<kv> (ctr_launch_render): the launch's buffers are cross-checked against the build, then
// up to three kernels go onto the stream — the first order of a new shape, the render, the fold of its counters and the
// next order (tile_order.hip).
// the scene head of the launch carries the record of the top-level walk's first leaf: the walk starts there without `meshes`
bool launch_head_mesh(const RenderLaunch &L) {
  return (L.head.mesh_dark & CTR_HEAD_MESH) != 0u && (L.scene.tlas_root & BVH_LEAF_FLAG) && L.scene.n_mesh != 0u;
}

int launch(const RenderLaunch &L, uint32_t kv, const void *kernel, hipStream_t stream) {
  KArgs A;
  const DScene &S = L.scene;
  A.objs = (const CADDR DObj *)S.objs;
  A.oloop = (const CADDR DObj *)S.oloop;
  A.meshes = (const CADDR DObj *)S.meshes;
  A.n_mesh = S.n_mesh;
  // "Scene head": the flags ride in words of the hot block the trip head has anyway
  A.head = L.head;
  const bool head_mesh = launch_head_mesh(L);
  const bool head_axis = L.head.n_axis_recs == 3u && S.n_axis_recs >= 3u && S.n_plane_recs >= 3u;
  A.tlas_root = S.tlas_root | (head_mesh ? CTR_TL_HEAD_FLAG : 0u);
  A.tlas_root2 = S.tlas_root_regular;
  A.tlas_begin = S.tlas_begin;
  for (int q = 0; q < 3; q++) { A.tl_mn[q] = S.tl_mn[q]; A.tl_mx[q] = S.tl_mx[q]; }
  A.planes = (const CADDR DPlanePair *)S.planes;
  A.n_oloop = S.n_oloop;
  A.n_plane_recs = S.n_plane_recs;
  A.n_axis_recs = S.n_axis_recs;
  A.tris = (const CADDR DTri *)S.tris;
  A.nodes = (const CADDR DNode *)S.nodes;
  A.nodes4 = (const CADDR DNode4 *)S.nodes4;
  A.gnorm = (const CADDR float *)S.gnorm;
  A.lights = (const CADDR DLight *)S.lights;
  A.mats = (const CADDR DMat *)S.mats;
  A.n_obj = S.n_obj;
  A.n_light = S.n_light;
  A.cams = (const CADDR DCam *)L.cams;
  A.w = L.w;
  A.h = L.h;
  A.first_frame = L.first_frame;
  A.n_frames = L.n_frames;
  A.frame_stride_px = L.frame_stride_px;
  A.rows = L.rows;
  A.fudge = L.fudge;
  A.bounces = L.bounces;
  A.has_mesh = (S.has_mesh ? 1u : 0u) | (head_axis ? 2u : 0u);
  const StackShape stack = stack_shape(L.bounces, S.any_bounce != 0, S.need_cold_frames != 0);
  A.nf = stack.nf;
  A.frames = stack.frames;
  A.order = (const CADDR uint32_t *)L.order;
  A.cost = L.cost;
  const bool host_delivery = (kv & KV_HOSTOUT) != 0;
  if (host_delivery != (L.group_done != nullptr)) return (int)hipErrorInvalidValue;
  if (host_delivery && (L.n_frames != 1 || !L.host_depth || !L.host_color || !L.host_normal)) return (int)hipErrorInvalidValue;
  A.host_depth = L.host_depth;
  A.host_color = L.host_color;
  A.host_normal = L.host_normal;
  A.group_done = L.group_done;
  A.uv_out = L.uv;
  if (((kv & KV_UV) != 0) != (L.uv != nullptr)) return (int)hipErrorInvalidValue;
  // "Supersampling": s = 2, 4 or 8 must divide the tile (a block of samples inside one wave) and the sample frame; one frame
  A.ss_log2 = (kv & KV_SS) ? L.ss_log2 : 0u;
  // "Lens render": the caller's rays, one pair per pixel (sample) of the one frame
  A.ray_origin = (kv & KV_RAYS) ? L.ray_origin : nullptr;
  A.ray_dir = (kv & KV_RAYS) ? L.ray_dir : nullptr;
  A.ray_ambient = (kv & KV_RAYS) ? L.ray_ambient : 0.f;
  if (((kv & KV_RAYS) != 0) != (L.ray_origin != nullptr) || ((kv & KV_RAYS) != 0) != (L.ray_dir != nullptr)) return (int)hipErrorInvalidValue;
  if ((kv & KV_RAYS) && L.n_frames != 1) return (int)hipErrorInvalidValue;
  if (((kv & KV_SS) != 0) != (L.ss_log2 != 0u)) return (int)hipErrorInvalidValue;
  if (kv & KV_SS) {
    const uint32_t m = (1u << L.ss_log2) - 1u;
    if (L.ss_log2 > 3u || ((TW | TH) & m) || ((L.w | L.h | L.rows.n_rows | L.rows.row_begin | L.rows.row_end | L.rows.block_rows) & m) || L.n_frames != 1)
      return (int)hipErrorInvalidValue;
  }
  size_t lds_bytes = (size_t)WAVES_PER_WG * lds_bytes_per_wave(kv, stack);  // (the stack, and PARK's 5 * 64 floats)
  // diagnostic only: extra dynamic LDS per workgroup caps the waves resident per CU (occupancy sweeps)
  if (const char *pad = getenv("CUTRACE_LDS_PAD")) lds_bytes += (size_t)atol(pad);
  const uint64_t waves = ctr_launch_waves(L);
  if (waves > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
  if (waves == 0) return 0;
  const uint32_t grid = (uint32_t)((waves + WAVES_PER_WG - 1) / WAVES_PER_WG);
  // counters go through the scene's shard buffer and are folded into the caller's words afterwards
  unsigned long long *shards = L.counters ? L.shards : nullptr;
  if (L.order_init && L.order) ctr_launch_first_order(L, stream);
  float *depth = L.depth, *color = L.color, *normal = L.normal;
  void *args[] = {&A, &depth, &color, &normal, &shards};  // render_kernel's parameter list (KParams)
  (void)hipLaunchKernel(kernel, dim3(grid), dim3(WG_THREADS), args, lds_bytes, stream);
  const bool reorder = L.cost && L.order_next;
  if (shards || reorder)
    ctr_launch_after_render(shards, L.counters, reorder ? L.cost : nullptr, L.order_next, (uint32_t)waves,
                            host_delivery ? tiles_x(L.w) : 0u, stream);
  return (int)hipGetLastError();
}

}  // namespace

// ---- self-test of norm_and_inverse against the library's correctly rounded sqrtf and division ----
namespace {
__global__ __launch_bounds__(256) void selftest_exact_math(unsigned long long *bad) {
  // every mantissa (2^23) x both exponent parities, at exponents -79/-78, -1/0 and 78/79: thread t takes 6 values
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;  // 0 .. 2^23-1
  unsigned long long wrong = 0;
  const int exps[6] = {127 - 79, 127 - 78, 126, 127, 127 + 78, 127 + 79};
  for (int k = 0; k < 6; k++) {
    float x = __uint_as_float(((uint32_t)exps[k] << 23) | m);
    asm volatile("" : "+v"(x));
    float n, inv;
    norm_and_inverse(x, n, inv);
    const float n_ref = sqrtf(x);
    const float inv_ref = 1.0f / n_ref;
    if (__float_as_uint(n) != __float_as_uint(n_ref) || __float_as_uint(inv) != __float_as_uint(inv_ref)) wrong++;
  }
  for (int off = 32; off > 0; off >>= 1) wrong += __shfl_xor(wrong, off);
  if ((threadIdx.x & 63) == 0 && wrong) atomicAdd(bad, wrong);
}
}  // namespace

#if defined(CTR_PROFILE)
// profile builds only (scripts/dynamic_mix.py): the 256 segment counters, optionally cleared
extern "C" int ctr_debug_profile_read(uint64_t *out256, int reset) {
  unsigned int h[256];
  if (hipDeviceSynchronize() != hipSuccess) return CTR_E_INVALID;
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof(h)) != hipSuccess) return CTR_E_INVALID;
  for (int q = 0; q < 256; q++) out256[q] = h[q];
  if (reset) {
    for (int q = 0; q < 256; q++) h[q] = 0u;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), h, sizeof(h)) != hipSuccess) return CTR_E_INVALID;
  }
  return CTR_OK;
}
#endif

// live-lane statistics of the CTR_VAR_STATS launches since the last reset (g_lane_stats above): 96 words
extern "C" int ctr_debug_lane_stats(uint64_t *out80, int reset) {
  if (!out80) return CTR_E_INVALID;
  unsigned long long h[96];
  if (hipDeviceSynchronize() != hipSuccess) return CTR_E_INVALID;
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lane_stats), sizeof(h)) != hipSuccess) return CTR_E_INVALID;
  for (int q = 0; q < 96; q++) out80[q] = h[q];
  if (reset) {
    for (int q = 0; q < 96; q++) h[q] = 0ull;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_lane_stats), h, sizeof(h)) != hipSuccess) return CTR_E_INVALID;
  }
  return CTR_OK;
}

extern "C" int ctr_selftest_exact_math(uint64_t *n_mismatch) {
  if (!n_mismatch) return CTR_E_INVALID;
  unsigned long long *d = nullptr;
  hipError_t e = hipMalloc((void **)&d, sizeof(unsigned long long));
  if (e != hipSuccess) return CTR_E_HIP_BASE + (int)e;
  (void)hipMemset(d, 0, sizeof(unsigned long long));
  hipLaunchKernelGGL(selftest_exact_math, dim3((1u << 23) / 256), dim3(256), 0, nullptr, d);
  unsigned long long h = ~0ull;
  e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return CTR_E_HIP_BASE + (int)e;
  *n_mismatch = h;
  return CTR_OK;
}

// The shape of the launch (kernel_choice.h launch_shape), from the facts that are final only here: the launch's scene head and
// root.  A head-held leaf of a scene with ONE mesh is that mesh's (the merged pseudo mesh, the other head-held leaf, belongs to
// KV_MERGE builds, which have no shape).
uint32_t ctr_launch_shape(const RenderLaunch &L) {
  if (L.no_shape) return KS_GENERAL;
  return launch_shape(L.variant, L.scene.n_oloop, launch_head_mesh(L) && L.scene.n_mesh == 1u);
}

// The opaque build of the launch (kernel_choice.h opaque_build), from its build and its shape.
uint32_t ctr_launch_opaque(const RenderLaunch &L) { return opaque_build(L.variant, ctr_launch_shape(L), L.no_opaque != 0u); }

// Whether the launch takes the phased twin of its opaque build (kernel_choice.h phased_build).
uint32_t ctr_launch_phased(const RenderLaunch &L) { return phased_build(ctr_launch_opaque(L), L.no_phase_split != 0u) ? 1u : 0u; }

// L.variant is the build (kernel_choice.h choose_kernel decides; launch cross-checks the launch's buffers against it).  The
// switch is what instantiates the kernels — and what makes a table entry listed twice a compile error.
int ctr_launch_render(const RenderLaunch &L, void *stream) {
  const void *kernel;
  switch (L.variant) {
#define X(kv) case (kv): kernel = (const void *)render_kernel<(kv)>; break;
    CTR_RENDER_KERNELS(X)
    CTR_LENS_KERNELS(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
  // the launch shape (kernel_choice.h): the same build, compiled for what this launch's scene cannot contain
  if (ctr_launch_shape(L) == KS_ONE_MESH) {
    const uint32_t opq = ctr_launch_opaque(L);
    // ... and, where the scene head carries room facts, with the code that uses them ("room-safe lanes"); and as the opaque
    // build the launch qualifies for ("opaque build")
    const bool room = L.head.room_lights != 0u;
    // ... and, an opaque build whose scene head carries the dark-skip fact, with the code that leaves those casts out ("dark lights")
    const bool dark = opq == KO_OPAQUE && (L.head.mesh_dark & CTR_HEAD_DARK) != 0u;
    // ... and an opaque build as its phased twin ("phased builds") unless the handle was created under CUTRACE_NO_PHASE_SPLIT=1
    const bool phased = ctr_launch_phased(L) != 0u;
    switch (L.variant) {
#define Y(kv, o, d, p) (room ? (const void *)render_kernel<(kv), KS_ONE_MESH, true, o, d, p> : (const void *)render_kernel<(kv), KS_ONE_MESH, false, o, d, p>)
#define Z(kv, d) (phased ? Y(kv, KO_OPAQUE, d, true) : Y(kv, KO_OPAQUE, d, false))
#define X(kv) case (kv): kernel = opq == KO_OPAQUE ? (dark ? Z(kv, true) : Z(kv, false)) : Y(kv, KO_PARENT, false, false); break;
      CTR_SHAPE_KERNELS(X)
#undef X
#undef Z
#undef Y
      default: return (int)hipErrorInvalidValue;
    }
  }
  return launch(L, L.variant, kernel, (hipStream_t)stream);
}
