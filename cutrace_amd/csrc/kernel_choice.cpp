// kernel_choice.cpp — choose_kernel: from the caller's CTR_VAR_* bits, the scene's facts and the entry point to the one build
// of CTR_RENDER_KERNELS (CTR_LENS_KERNELS for the lens entries) the launch gets, or to the reason why there is none (kernel_choice.h).
// launch_shape: which launch shape of that build a launch gets, from two facts of its scene.
#include "kernel_choice.h"

#include "cutrace_amd.h"

KernelChoice choose_kernel(const KernelFacts &f) {
  const uint32_t u = f.user;
  const bool lens = f.entry == KE_DEVICE_LENS || f.entry == KE_DEVICE_LENS_SS;
  if (lens && (u & (CTR_VAR_STATS | CTR_VAR_IGNORE_TRANSPARENT | CTR_VAR_NO_PREFILTER | CTR_VAR_NO_CLUSTER))) return {0, false, false, KR_LENS};
  const bool ss = f.entry == KE_HOST_SS || f.entry == KE_DEVICE_SS;
  if (ss && (u & (CTR_VAR_STATS | CTR_VAR_IGNORE_TRANSPARENT | CTR_VAR_NO_PREFILTER | CTR_VAR_NO_CLUSTER))) return {0, false, false, KR_SS};
  if (f.entry == KE_DEVICE && (u & CTR_VAR_IGNORE_TRANSPARENT)) return {0, false, false, KR_IGNTR_DEVICE};
  // the counting launch walks like the reference, whatever else is asked for
  if (f.entry == KE_COUNT) return {KV_PREFILTER | KV_COUNT, false, false, KR_NONE};
  const bool igntr = (u & CTR_VAR_IGNORE_TRANSPARENT) != 0;  // (KE_HOST, KE_UV: the others have left)
  const bool uv = f.entry == KE_UV || igntr;
  const bool stats = (u & CTR_VAR_STATS) != 0;
  if (uv && stats) return {0, false, false, KR_UV_STATS};

  constexpr uint32_t SHIPPED = KV_PREFILTER | KV_BVH;
  const uint32_t walk = (u & CTR_VAR_NO_PREFILTER ? 0u : KV_PREFILTER) | (u & CTR_VAR_NO_CLUSTER ? 0u : KV_BVH);
  // shadow any-hit is result-identical only when every material is exactly opaque; with any transparency the ordered
  // nearest-hit loop is kept
  const uint32_t anyhit = f.all_opaque && !(u & CTR_VAR_NO_ANYHIT) ? KV_ANYHIT : 0u;
  // the fast specular path: unless the caller wants the exact one, or the scene's exponents and colours would take it out of
  // the colour tolerance (then the launch is the one CTR_VAR_EXACT_POW would get)
  const uint32_t pow = (u & CTR_VAR_EXACT_POW) || !f.fast_pow_ok ? 0u : KV_FASTPOW;
  // the build for 6 waves per SIMD: for large meshes, of the default variant only, and only when the stacks leave it room
  const uint32_t occ6 = f.big_mesh && !(u & CTR_VAR_NO_OCC6) && walk == SHIPPED && anyhit && pow && occ6_fits(f.stack) ? KV_OCC6 : 0u;

  // the fourth output and the supersampled frame: the shipped walk only, through device buffers
  if (uv) return {SHIPPED | KV_UV | (igntr ? KV_IGNTR : 0u) | anyhit | pow, false, false, KR_NONE};
  if (ss) return {SHIPPED | KV_SS | anyhit | pow | occ6, false, false, KR_NONE};
  // the caller's primary rays: the same, with or without the in-kernel reduction
  if (lens) return {SHIPPED | KV_RAYS | (f.entry == KE_DEVICE_LENS_SS ? KV_SS : 0u) | anyhit | pow | occ6, false, false, KR_NONE};
  // KE_HOST, KE_DEVICE.  The merged tree (CTR_VAR_MERGE): a walk of the shipped kind, frame leaving through device buffers
  const bool merged = (u & CTR_VAR_MERGE) && f.merged_usable && (stats || walk == SHIPPED);
  const uint32_t merge = merged ? KV_MERGE : 0u;
  // the statistics build is the shipped walk with fast pow, whatever else is asked for
  if (stats) return {SHIPPED | KV_FASTPOW | KV_STATS | anyhit | merge, false, merged, KR_NONE};
  // delivery by the kernel: for the variants the library picks by itself, not for the ablation builds
  const bool direct = f.entry == KE_HOST && f.deliverable && !merged && !(u & CTR_VAR_NO_DIRECT) && walk == SHIPPED && pow;
  return {walk | anyhit | pow | occ6 | merge | (direct ? KV_HOSTOUT : 0u), direct, merged, KR_NONE};
}

uint32_t opaque_build(uint32_t kv, uint32_t shape, bool no_opaque) {
  return !no_opaque && shape == KS_ONE_MESH && (kv & KV_ANYHIT) ? KO_OPAQUE : KO_PARENT;
}

bool phased_build(uint32_t opq, bool no_phase_split) { return !no_phase_split && opq == KO_OPAQUE; }

uint32_t launch_shape(uint32_t kv, uint32_t n_oloop, bool head_mesh) {
  if (!head_mesh || n_oloop != 0u) return KS_GENERAL;
  switch (kv) {
#define X(k) case (k):
    CTR_SHAPE_KERNELS(X)
#undef X
    return KS_ONE_MESH;
    default: return KS_GENERAL;
  }
}
