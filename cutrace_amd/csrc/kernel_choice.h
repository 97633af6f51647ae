// kernel_choice.h — which build of render_kernel<KV> a launch gets: the list of builds, the stack shape of a launch, and the
// ONE function that knows which combination of caller's wishes, scene facts and entry point has a build.
//
// Host only, no HIP: ctr_render.cpp asks choose_kernel() and hands the answer to ctr_launch_render (render_kernel.hip), whose
// switch is generated from the same list; scripts/kernel_choice_check.cpp prints the answer for the whole input space.
#ifndef CUTRACE_AMD_KERNEL_CHOICE_H
#define CUTRACE_AMD_KERNEL_CHOICE_H

#include <stddef.h>
#include <stdint.h>

#include "scene_device.h"

// Every instantiation of render_kernel, once.  A family is a fixed set of bits plus the optional bits it honours; what a
// family does not list it ignores (the shipped walk is KV_PREFILTER | KV_BVH).
#define CTR_RENDER_KERNELS(X)                                                                                                  \
  /* main walk: KV_PREFILTER, KV_ANYHIT, KV_BVH, KV_FASTPOW, each on or off */                                                 \
  X(0u) X(KV_PREFILTER) X(KV_ANYHIT) X(KV_PREFILTER | KV_ANYHIT)                                                               \
  X(KV_BVH) X(KV_BVH | KV_PREFILTER) X(KV_BVH | KV_ANYHIT) X(KV_BVH | KV_PREFILTER | KV_ANYHIT)                                \
  X(KV_FASTPOW) X(KV_FASTPOW | KV_PREFILTER) X(KV_FASTPOW | KV_ANYHIT) X(KV_FASTPOW | KV_PREFILTER | KV_ANYHIT)                \
  X(KV_FASTPOW | KV_BVH) X(KV_FASTPOW | KV_BVH | KV_PREFILTER) X(KV_FASTPOW | KV_BVH | KV_ANYHIT)                              \
  X(KV_FASTPOW | KV_BVH | KV_PREFILTER | KV_ANYHIT)                                                                            \
  /* 6-wave: the default variant only (shipped walk, any-hit, fast pow); no optional bit */                                    \
  X(KV_OCC6 | KV_PREFILTER | KV_ANYHIT | KV_BVH | KV_FASTPOW)                                                                  \
  /* host delivery: shipped walk, fast pow; honours KV_ANYHIT, and with it KV_OCC6 */                                          \
  X(KV_PREFILTER | KV_BVH | KV_FASTPOW | KV_HOSTOUT) X(KV_PREFILTER | KV_BVH | KV_FASTPOW | KV_HOSTOUT | KV_ANYHIT)            \
  X(KV_PREFILTER | KV_BVH | KV_FASTPOW | KV_HOSTOUT | KV_ANYHIT | KV_OCC6)                                                     \
  /* STATS: shipped walk, fast pow; honours KV_ANYHIT */                                                                       \
  X(KV_BVH | KV_PREFILTER | KV_FASTPOW | KV_STATS) X(KV_BVH | KV_PREFILTER | KV_ANYHIT | KV_FASTPOW | KV_STATS)                \
  /* COUNT: the reference's walk with the prefilter; no optional bit */                                                        \
  X(KV_PREFILTER | KV_COUNT)                                                                                                   \
  /* UV: shipped walk; honours KV_ANYHIT, KV_FASTPOW */                                                                        \
  X(KV_PREFILTER | KV_BVH | KV_UV) X(KV_PREFILTER | KV_BVH | KV_UV | KV_ANYHIT)                                                \
  X(KV_PREFILTER | KV_BVH | KV_UV | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_UV | KV_FASTPOW | KV_ANYHIT)                      \
  /* UV + IGNTR: as UV */                                                                                                      \
  X(KV_PREFILTER | KV_BVH | KV_UV | KV_IGNTR) X(KV_PREFILTER | KV_BVH | KV_UV | KV_IGNTR | KV_ANYHIT)                          \
  X(KV_PREFILTER | KV_BVH | KV_UV | KV_IGNTR | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_UV | KV_IGNTR | KV_FASTPOW | KV_ANYHIT) \
  /* MERGE: shipped walk; honours KV_ANYHIT, KV_FASTPOW, with both KV_OCC6, and KV_STATS (then fast pow, no 6-wave) */         \
  X(KV_PREFILTER | KV_BVH | KV_MERGE) X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_ANYHIT)                                          \
  X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_FASTPOW | KV_ANYHIT)                \
  X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_FASTPOW | KV_ANYHIT | KV_OCC6)                                                       \
  X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_FASTPOW | KV_STATS) X(KV_PREFILTER | KV_BVH | KV_MERGE | KV_ANYHIT | KV_FASTPOW | KV_STATS) \
  /* SS: shipped walk; honours KV_ANYHIT, KV_FASTPOW, and with both KV_OCC6 */                                                 \
  X(KV_PREFILTER | KV_BVH | KV_SS) X(KV_PREFILTER | KV_BVH | KV_SS | KV_ANYHIT)                                                \
  X(KV_PREFILTER | KV_BVH | KV_SS | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_SS | KV_FASTPOW | KV_ANYHIT)                      \
  X(KV_PREFILTER | KV_BVH | KV_SS | KV_FASTPOW | KV_ANYHIT | KV_OCC6)

// The builds of the lens render (caller-supplied primary rays, KV_RAYS), a list of their own beside the first: ctr_launch_render's
// switch is generated from both, and choose_kernel returns one of THESE for KE_DEVICE_LENS / KE_DEVICE_LENS_SS only.
#define CTR_LENS_KERNELS(X)                                                                                                    \
  /* RAYS: shipped walk; honours KV_ANYHIT, KV_FASTPOW, and with both KV_OCC6 */                                               \
  X(KV_PREFILTER | KV_BVH | KV_RAYS) X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_ANYHIT)                                            \
  X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_FASTPOW | KV_ANYHIT)                  \
  X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_FASTPOW | KV_ANYHIT | KV_OCC6)                                                        \
  /* RAYS + SS: as RAYS */                                                                                                     \
  X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_SS) X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_SS | KV_ANYHIT)                            \
  X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_SS | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_SS | KV_FASTPOW | KV_ANYHIT)  \
  X(KV_PREFILTER | KV_BVH | KV_RAYS | KV_SS | KV_FASTPOW | KV_ANYHIT | KV_OCC6)

// The launch shape: a second template parameter of render_kernel<KV, SHAPE> beside the build, decided per LAUNCH from facts of the
// scene the build does not depend on (launch_shape below).  It is not a KV bit: choose_kernel, KernelChoice::kv and
// ctr_debug_last_kernel say what they said before there were shapes (ctr_debug_last_shape reads the shape back).
//   KS_GENERAL  : any scene.
//   KS_ONE_MESH : no sphere and no stand-alone triangle, and exactly one mesh whose record rides in the scene head
//                 (scene_device.h DSceneHead::mesh): the object loop and the top-level walk are compiled out.  Only code that
//                 such a scene never runs is removed, so every result has the same bits.
enum : uint32_t { KS_GENERAL = 0u, KS_ONE_MESH = 1u };
// The builds that exist in shape KS_ONE_MESH, a list of their own: the default variant (shipped walk, any-hit, fast pow), with
// or without the 6-wave build, with or without host delivery.  Each is also in CTR_RENDER_KERNELS (its KS_GENERAL twin).
#define CTR_SHAPE_KERNELS(X)                                                                                                   \
  X(KV_PREFILTER | KV_BVH | KV_ANYHIT | KV_FASTPOW) X(KV_PREFILTER | KV_BVH | KV_ANYHIT | KV_FASTPOW | KV_OCC6)                \
  X(KV_PREFILTER | KV_BVH | KV_ANYHIT | KV_FASTPOW | KV_HOSTOUT) X(KV_PREFILTER | KV_BVH | KV_ANYHIT | KV_FASTPOW | KV_HOSTOUT | KV_OCC6)
// The shape of a launch of build `kv`: n_oloop = spheres and stand-alone triangles of the scene (DScene::n_oloop), head_mesh =
// the launch's scene head carries the record of the scene's only mesh (render_kernel.hip launch).  KS_ONE_MESH for the builds
// of CTR_SHAPE_KERNELS with n_oloop == 0 and head_mesh, KS_GENERAL for everything else.
uint32_t launch_shape(uint32_t kv, uint32_t n_oloop, bool head_mesh);

// The opaque build: a fourth template parameter of render_kernel<KV, SHAPE, ROOM, OPQ>, decided per LAUNCH like the shape and, like
// it, not a KV bit (ctr_debug_last_opaque reads it back).  An any-hit build runs only when every material is exactly opaque
// (choose_kernel), so ray_color's pass-through half never runs in it; the opaque builds of the one-mesh shape compile it out.
//   KO_PARENT : the code as it was.
//   KO_OPAQUE : no pass-through state in the continuation; the hit point lives in the ray origin alone.
enum : uint32_t { KO_PARENT = 0u, KO_OPAQUE = 1u };
// The opaque build of a launch of build `kv` in shape `shape` (launch_shape); no_opaque: the handle was created under
// CUTRACE_NO_OPAQUE_BUILD=1.  KO_OPAQUE when the shape is KS_ONE_MESH and the build any-hit (every build of CTR_SHAPE_KERNELS
// is), KO_PARENT for everything else.  The stack plays no part: an opaque build asks for the LDS of its parent twin.
uint32_t opaque_build(uint32_t kv, uint32_t shape, bool no_opaque);

// The phased build: a sixth template parameter of render_kernel<KV, SHAPE, ROOM, OPQ, DARK, PHASED>, decided per LAUNCH like the
// opaque build and, like it, not a KV bit (ctr_debug_last_phased reads it back).  In an opaque build all active lanes of a wave
// cast for the same reason and towards the same light in every trip (render_kernel.hip "Phased builds"); the phased twin of an
// opaque build keeps that as scalar state and compiles a radiance trip and a shadow trip apart.
// The phased build of a launch whose opaque build is `opq` (opaque_build); no_phase_split: the handle was created under
// CUTRACE_NO_PHASE_SPLIT=1.  True exactly when opq is KO_OPAQUE and the switch is unset.
bool phased_build(uint32_t opq, bool no_phase_split);

// The recursion stack of a launch: `frames` frames of `nf` floats per lane (render_kernel.hip KArgs::frames, ::nf).
struct StackShape {
  uint32_t frames, nf;
  size_t bytes_per_wave() const { return (size_t)frames * nf * 64 * sizeof(float); }
};
// need_cold: some material both reflects and transmits; any_bounce: some material does either (only then does ray_color recurse)
inline StackShape stack_shape(int bounces, bool any_bounce, bool need_cold) {
  return {(uint32_t)((bounces > 0 && any_bounce) ? bounces : 1), need_cold ? 10u : 4u};
}
// The 6-waves-per-SIMD build parks 1280 bytes of shading state per wave in LDS (render_kernel PARK); LDS is handed out
// in granules of 1280 bytes (160 KB / 128), and 24 waves per CU need at most 5 granules each: bounces <= 5 without cold frames
inline bool occ6_fits(StackShape st) { return (st.bytes_per_wave() + 1280u + 1279u) / 1280u <= 5u; }
// dynamic LDS of one wave of a launch of build `kv`, in any shape and as the opaque build or not: its stack, and the parking
// granule of the 6-wave builds
inline size_t lds_bytes_per_wave(uint32_t kv, StackShape st) { return st.bytes_per_wave() + ((kv & KV_OCC6) ? 1280u : 0u); }

enum KernelEntry {
  KE_HOST,       // ctr_render
  KE_COUNT,      // ctr_algorithmic_bytes
  KE_UV,         // ctr_render_uv
  KE_HOST_SS,    // ctr_render_aa
  KE_DEVICE,     // ctr_render_device, ctr_render_device_batch
  KE_DEVICE_SS,  // ctr_render_device_aa
  KE_DEVICE_LENS,     // ctr_render_device_lens, samples == 1
  KE_DEVICE_LENS_SS,  // ctr_render_device_lens, samples > 1
};
enum KernelReject {
  KR_NONE,
  KR_SS,             // supersampling has no build for the caller's variant bits
  KR_UV_STATS,       // the fourth output / ignore_transparent cast has no statistics build
  KR_IGNTR_DEVICE,   // CTR_VAR_IGNORE_TRANSPARENT is for host-buffer calls
  KR_LENS,           // the lens render has no build for the caller's variant bits
};
struct KernelFacts {
  uint32_t user;        // CTR_VAR_* of the handle
  bool all_opaque;      // every material exactly opaque: shadow any-hit is result-identical
  bool big_mesh;        // mesh triangles >= ctr_scene::occ6_min_tris()
  bool merged_usable;   // the merged tree is built and nothing speaks against walking it (scene_flatten.h Merged)
  KernelEntry entry;
  bool deliverable;     // KE_HOST: the caller's buffers are page-locked and visible to the device
  StackShape stack;
  bool fast_pow_ok = true;  // the fast specular path stays inside the colour tolerance on this scene (scene_flatten.h fast_pow_in_bar)
};
struct KernelChoice {
  uint32_t kv;          // the build, one of CTR_RENDER_KERNELS — of CTR_LENS_KERNELS for the lens entries — (reject == KR_NONE)
  bool direct;          // the kernel delivers the frame to the caller's buffers itself (KV_HOSTOUT)
  bool merged;          // the top-level root is the merged pseudo mesh (KV_MERGE)
  KernelReject reject;
};
KernelChoice choose_kernel(const KernelFacts &f);

#endif
