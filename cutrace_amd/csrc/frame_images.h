// frame_images.h — what ctr_quantise_device and ctr_render_images (ctr_render.cpp) hand the quantise kernel (frame_images.hip).
#ifndef CUTRACE_AMD_FRAME_IMAGES_H
#define CUTRACE_AMD_FRAME_IMAGES_H

#include <stdint.h>

// the planes of include/cutrace_images.h ctr_image_planes, checked: a plane is present where its output is non-null
struct ImagesLaunch {
  uint64_t n;                                  // pixels
  const float *depth, *color, *normal;         // n, 3n, 3n floats, 4-byte aligned
  uint8_t *depth8, *color8, *normal8;          // 3n bytes each, any alignment
  const unsigned long long *counters;          // non-null: max depth = the float whose bits are the low half of word [1]
  float max_depth;                             // else
};

// host-callable launcher implemented in frame_images.hip; returns a hipError_t as int
int ctr_launch_images(const ImagesLaunch &L, void *stream);

#endif
