/*
 * cutrace_lens.h — the lens render: the render kernel on caller-supplied primary rays, one (origin, direction) per pixel or
 * per sample.  A fisheye, a stereo pair, a distorted lens, a thin lens with jittered samples or stochastic anti-aliasing
 * run on the wave-uniform walk of ctr_render_device (one wave walks one 8x8 tile together), keep its tile scheduler and,
 * with `samples`, the in-kernel box filter of cutrace_aa.h.  ctr_shade_rays (cutrace_rays.h) stays the call for rays in no
 * particular order.
 *
 * Definition.  The lens frame has the scene's current size w x h (ctr_scene_size); with samples = s in {2, 4, 8} it is the
 * s*w x s*h SAMPLE frame.  d_origin and d_dir hold 3 floats per pixel (sample), row-major over the WHOLE (sample) frame:
 * n_rays = s*s*w*h, indexed by the global image row also when `rows` selects a part.  Outputs are compact, as in
 * ctr_render_device.
 *
 *   Pixel (sample) (x, y) holds what the plain render holds, for the ray {origin, dir.normalized()} in place of
 *   cam::get_ray(x, y): depth and normal from ray_cast, colour from ray_color<bounces>(scene, ray, fudge, ambient);
 *   normalized() is the reference's v * (1.0f / sqrtf(x*x + y*y + z*z)) (inc/vector.hpp).  The duplicated primary cast
 *   counts twice in ray_count, as in every render.  `ambient` is an argument of the call (the plain render passes the
 *   camera's).  Normalising keeps every cast in the near-unit regime the render's box margins and reciprocal clamps were
 *   derived in.
 *
 *   Masked rays.  A ray is masked when its origin has a non-finite component, or when its NORMALISED direction has a
 *   non-finite component or is (0, 0, 0) — which covers NaN, infinite and zero directions and directions whose squared
 *   length leaves the float range.  A masked pixel makes no cast, is not counted in ray_count, receives the miss values
 *   (depth +inf, normal 0, colour 0) and does not enter max_depth: the way to say "no ray here", e.g. outside a fisheye's
 *   image circle.
 *
 *   samples = s > 1.  The frame is the lens render of the s*w x s*h rays reduced exactly as ctr_render_device_aa reduces
 *   (cutrace_aa.h): depth and normal of pixel (x, y) are those of sample (s*x, s*y) — the miss values when that sample is
 *   masked —, the colour is the float32 halving tree along x, then along y, times 1.0f / (s*s); a masked sample contributes
 *   (0, 0, 0).
 *
 * Exactness.  As for every BVH walk of the library: the guard records protect the scene's eyes, its lights
 * and their mirror images, not arbitrary origins.  A lens ray that lies in the plane of a mesh triangle to rounding may
 * differ from the reference's linear walk; ctr_shade_rays with CTR_SHADE_LINEAR remains the exact call.
 *
 * Contract: ctr_render_device's.  Asynchronous on `hip_stream`, no synchronisation; allocates only on the first launch of a
 * shape (capturable into a graph after that launch, or under CTR_VAR_NO_REORDER); d_counters accumulated into ([0]
 * ray_count, [1] max-depth bits).  The rays must stay valid and unchanged until the launch has run.
 *
 * Tile scheduling (cutrace_amd.h): the learned order is keyed by the launch's shape, which holds w and h but not where the
 * rays come from.  A lens launch therefore shares the learned order of the plain launch of the same size (and a lens launch
 * with samples = s that of ctr_render_device_aa with s), and the other way round.  Results never depend on the order.
 *
 * Variant bits (ctr_set_variant): CTR_VAR_NO_ANYHIT, CTR_VAR_EXACT_POW, CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST and
 * CTR_VAR_NO_OCC6 are honoured; CTR_VAR_MERGE and CTR_VAR_NO_DIRECT have nothing to act on and are ignored.  CTR_VAR_STATS,
 * CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER and CTR_VAR_NO_CLUSTER have no lens build: the call fails.
 *
 * The call returns CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for: a NULL scene, lens, ray
 * array or output buffer; samples not in {1, 2, 4, 8}; n_rays != samples^2 * w * h; with samples > 1, s*w or s*h beyond
 * uint32 or a sample frame of more than 0x7FFFFFFF tiles; ray arrays that are not device memory of the scene's device; one
 * of the four variant bits above.  There is no host-buffer form: the rays are device data.  CTR_ABI_VERSION is unchanged.
 */
#ifndef CUTRACE_LENS_H
#define CUTRACE_LENS_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctr_lens {
  uint64_t n_rays;        /* must equal samples^2 * w * h of the scene's current size */
  uint32_t samples;       /* 1, 2, 4 or 8 per axis */
  float ambient;          /* phong's ambient factor (the plain render passes the camera's) */
  const float *d_origin;  /* n_rays x 3, device memory of the scene's device */
  const float *d_dir;     /* n_rays x 3, need not be normalised */
} ctr_lens;

int ctr_render_device_lens(ctr_scene *scene, float fudge, int bounces, const ctr_lens *lens, const ctr_rows *rows,
                           void *d_depth, void *d_color3, void *d_normal3, void *d_counters, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
