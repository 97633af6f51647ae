/*
 * cutrace_images.h — display frames: colour, depth and normal quantised to 8 bits on the GPU.
 *
 * The reference writes three 8-bit pictures of a frame (inc/images.hpp:26-88); the host library restates its three
 * quantisation rules as ctr_quantise_depth / _normal / _color (cutrace_host.h).  The calls below apply the same rules on the
 * device, so that 9 bytes per pixel leave the GPU instead of 28, and a frame that stays on the GPU (ctr_render_device*,
 * ctr_render_device_lens) can be turned into display bytes there.
 *
 * Definition.  Every plane is 3 bytes per pixel, R G B interleaved; depth is replicated to R = G = B.  Each float operation
 * below is rounded once (no fused multiply-add), every conversion to a byte truncates toward zero:
 *   depth   v finite ? (byte)((255.0f * (max_d - v)) / max_d) : 0                   (IEEE division)
 *   normal  len = sqrtf((x*x + y*y) + z*z);  (double)len <= 1e-6 ? (0, 0, 0)
 *           : f = 1.0f / len, per component c: (byte)(255.0f * (0.5f + 0.5f * (f * c)))
 *   colour  lo = (0.0f < v) ? v : 0.0f;  c = (lo < 1.0f) ? lo : 1.0f;  (byte)(255.0f * c)   — NaN gives 0, +inf 255
 * For every input on which the host quantisers are defined, the bytes are theirs, bit for bit.
 *
 * Saturation.  The host's C++ leaves the conversion of a float outside [0, 256) to a byte undefined.  That happens for a NaN
 * or infinite normal, a finite depth below 0 or above max_d, max_d == 0 with a finite depth, and a product that overflows.
 * Here the conversion is defined for every bit pattern: the float is clamped to [0, 255] first and NaN gives 0.  So
 *   depth   v > max_d -> 0;  v < 0 -> 255;  max_d == 0: v == 0 -> 0 (0/0), v < 0 -> 255 (+inf), v > 0 -> 0 (-inf)
 *   normal  a NaN component or a NaN length -> 0 for every component it reaches;  an infinite component -> length +inf,
 *           f = 0: the infinite component gives 0 (0 * inf), the finite ones 127
 * No input makes the kernel fault.
 *
 * max_d is the frame's largest finite depth (ctr_render_stats.max_depth) — the reason why depth bytes cannot be made
 * tile by tile inside the render kernel: they need the whole frame's maximum.  It is either passed as a float or read ON THE
 * DEVICE from the counter block a device-form render accumulated into (d_counters: the float's bits are the low 32 bits of
 * word [1]), so that render and quantise chain on one stream without a host round trip.
 */
#ifndef CUTRACE_IMAGES_H
#define CUTRACE_IMAGES_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctr_image_planes {
  uint64_t n_pixels;            /* 0: nothing is launched */
  const float *d_depth, *d_color3, *d_normal3;   /* device, n / 3n / 3n floats; NULL = plane absent */
  uint8_t *d_depth8, *d_color8, *d_normal8;      /* device, 3n bytes each; NULL exactly where the input is */
  const void *d_counters;       /* non-NULL: max depth = float bits in the low half of word [1], read on the device */
  float max_depth;              /* used when d_counters is NULL */
  uint32_t reserved;            /* 0 */
} ctr_image_planes;

/* Quantise n_pixels pixels of the planes that are present.  Asynchronous on `hip_stream`; allocates nothing and never
 * synchronises (capturable into a graph as one link of a linear chain).  Inputs need 4-byte alignment only, outputs none.
 * CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for: a NULL p; a non-zero `reserved`; an input
 * without its output or an output without its input; no plane at all; a pointer (d_counters included) that is not device
 * memory of `device`. */
int ctr_quantise_device(int device, const ctr_image_planes *p, void *hip_stream);

/* Host form, ctr_render's contract (synchronous; rows and stats as there, stats.max_depth what ctr_render reports for the
 * same call; samples 1, 2, 4 or 8 as in ctr_render_aa, cutrace_aa.h): the selected rows are rendered into the handle's own
 * device block, quantised there with the call's own largest depth, and only the requested byte planes — rows*w*3 bytes
 * each, any of them may be NULL, not all three — are copied out, one transfer per plane (asynchronous where the
 * destination is page-locked).  The variants ctr_render_aa rejects are rejected with samples > 1, with its messages;
 * CTR_VAR_IGNORE_TRANSPARENT with samples == 1 is honoured as in ctr_render. */
int ctr_render_images(ctr_scene *scene, float fudge, int bounces, uint32_t samples, const ctr_rows *rows,
                      uint8_t *depth8, uint8_t *color8, uint8_t *normal8, ctr_render_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
