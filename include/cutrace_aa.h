/*
 * cutrace_aa.h — the supersampled render: s x s samples per pixel (s = 1, 2, 4 or 8), box-filtered inside the kernel.
 *
 * The reference shoots one ray through each pixel's corner: cam::get_ray(x, y) is
 *   ((float)x / (float)w - 0.5f) * aspect * right + (0.5f - (float)y / (float)h) * up + forward,   aspect = (float)w / (float)h
 * (inc/default_schema.hpp:376-386), no pixel-centre offset.  For s a power of two, (float)(s*x) / (float)(s*w) equals
 * (float)x / (float)w bit for bit, and so does the aspect.  Hence the definition, which is the reference's own:
 *
 *   The supersampled w x h frame is the reference's render of the same scene at s*w x s*h, reduced block by block:
 *   sample (sx, sy) of pixel (x, y) is the big frame's pixel (s*x + sx, s*y + sy).
 *     depth, normal   those of sample (0, 0): bit for bit the buffers of the plain w x h render (ctr_render), and
 *                     stats.max_depth with them
 *     colour          the mean of the s*s samples' ray_color, summed in float32 in this fixed order:
 *                       1. along x by repeated halving, a[i] = a[2i] + a[2i+1], until one value per sample row is left;
 *                       2. along y in the same way;
 *                       3. multiplied by 1.0f / (s*s).
 *                     (the sum of two floats does not depend on the operands' order, so the order of a pair is free)
 *     samples = 1     ctr_render / ctr_render_device, bit for bit (the call is forwarded)
 *
 * The kernel renders the s*w x s*h samples — one wave is one 8x8 tile of them, so a block of samples always lies inside
 * one wave — and reduces each block across the lanes at the end of the wave: nothing goes through memory, and the frame
 * that leaves the chip is the w x h one.
 *
 * rows, the output buffers and stats.rows are in OUTPUT pixels (the row selection ((y / block_rows) % n_parts) == part
 * is applied to output rows).  stats.ray_count is the reference's cast count for the s*w x s*h frame.
 *
 * Tile scheduling (cutrace_amd.h): an AA launch is a launch of the shape s*w x s*h, the plain launch one of w x h.  A
 * handle keeps ONE learned tile order, so a handle that alternates plain and AA launches (or two values of `samples`)
 * relearns its order each time — every such launch runs in first-launch order and, in the device form, the first
 * launch of the larger shape allocates the cost / order buffers.  Results never depend on the order.
 *
 * Variant bits (ctr_set_variant): CTR_VAR_NO_ANYHIT, CTR_VAR_EXACT_POW, CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST and
 * CTR_VAR_NO_OCC6 are honoured; CTR_VAR_MERGE and CTR_VAR_NO_DIRECT have nothing to act on (the supersampled frame always
 * leaves through device buffers and a copy, the walk is the two-level one) and are ignored.  The ablation and diagnostic
 * builds have no supersampled variant: CTR_VAR_STATS, CTR_VAR_IGNORE_TRANSPARENT, CTR_VAR_NO_PREFILTER and
 * CTR_VAR_NO_CLUSTER on the handle make both calls fail.
 *
 * Both calls return CTR_E_INVALID, with a ctr_last_error message, before the GPU is touched, for: a NULL scene; samples
 * not in {1, 2, 4, 8}; s*w or s*h beyond uint32, or a sample frame of more than 0x7FFFFFFF tiles; one of the four variant
 * bits above.
 */
#ifndef CUTRACE_AA_H
#define CUTRACE_AA_H

#include <stdint.h>

#include "cutrace_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-buffer form: ctr_render's contract (synchronous; depth rows*w floats, color3 / normal3 rows*w*3 floats).
 * samples: 1, 2, 4 or 8 per axis. */
int ctr_render_aa(ctr_scene *scene, float fudge, int bounces, uint32_t samples, const ctr_rows *rows,
                  float *depth, float *color3, float *normal3, ctr_render_stats *stats);

/* Device-buffer form: ctr_render_device's contract — asynchronous on `hip_stream`, no synchronisation, no allocation
 * after a shape's first launch (capturable into a graph after that launch, or under CTR_VAR_NO_REORDER), d_counters
 * accumulated into ([0] ray_count of the s*w x s*h frame, [1] max-depth bits). */
int ctr_render_device_aa(ctr_scene *scene, float fudge, int bounces, uint32_t samples, const ctr_rows *rows,
                         void *d_depth, void *d_color3, void *d_normal3, void *d_counters, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif
