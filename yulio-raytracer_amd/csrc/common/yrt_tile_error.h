// yrt_tile_error.h — the error estimate of a 16x16 tile that adaptive sampling stops tiles by.
//
// After Dammertz, Hanika, Keller and Lensch, "A hierarchical automatic stopping condition for
// Monte Carlo global illumination" (2010): the frame's running sums S (weight w, every iteration)
// are compared with the sums H (weight h) of every second iteration, the "half buffer". Per pixel
//   I_c = S_c * rcp(w),  A_c = H_c * rcp(h)                     (c = r, g, b; linear radiance)
//   d   = (|I_r - A_r| + |I_g - A_g|) + |I_b - A_b|
//   s   = (I_r + I_g) + I_b
//   e   = s > 0 ? d * rsqrt(s) : 0
// and per tile E_T = (sum of its 256 slots) * rcp(n_T): the slots in scan order (slot = dy * 16 +
// dx), pixels outside the image 0, n_T the tile's pixels inside the image, the sum a fixed pairwise
// tree (slot i += slot i + h for h = 128, 64, ... 1). A NaN e (a non-finite sum) makes E_T NaN,
// which is below no threshold.
//
// Stated once for the device (k_tile_error, kernels/k_adaptive.h: one slot per thread, the tree in
// LDS) and the host (yrt_tile_error below, yrtDebugTileError), with operations that give the same
// bits on both: + - * |.| and the reference's rcp / rsqrt (yrt_sse_rcp.h); no IEEE division, no
// sqrtf. Both sides are compiled without FMA contraction.
#pragma once

#include "yrt_sse_rcp.h"

#define YRT_TILE_ERROR_SLOTS 256

// one pixel: S = (sum.rgb, w), H = (half sum.rgb, h)
YRT_SSE_FN float yrt_pixel_error(const float* S, const float* H) {
  const float rw = yrt_ref_rcp(S[3]), rh = yrt_ref_rcp(H[3]);
  const float Ir = S[0] * rw, Ig = S[1] * rw, Ib = S[2] * rw;
  const float Ar = H[0] * rh, Ag = H[1] * rh, Ab = H[2] * rh;
  const float d = (__builtin_fabsf(Ir - Ar) + __builtin_fabsf(Ig - Ag)) + __builtin_fabsf(Ib - Ab);
  const float s = (Ir + Ig) + Ib;
  return s > 0.0f ? d * yrt_ref_rsqrt(s) : 0.0f;
}

// one step of the tree for slot i < h: the device runs the slots of a step side by side
YRT_SSE_FN void yrt_tile_tree_step(float* slots, int i, int h) { slots[i] = slots[i] + slots[i + h]; }

// the pixels of image tile (tx, ty) that lie inside the width x height image
YRT_SSE_FN int yrt_tile_pixels(int tx, int ty, int width, int height) {
  const int nx = width - tx * 16 < 16 ? width - tx * 16 : 16;
  const int ny = height - ty * 16 < 16 ? height - ty * 16 : 16;
  return nx * ny;
}

// E_T from the tree's root
YRT_SSE_FN float yrt_tile_error_mean(float sum, int pixels) { return sum * yrt_ref_rcp((float)pixels); }

// The whole estimate of image tile (tx, ty), serially: accu4 / half4 are [height][width][4] floats.
YRT_SSE_FN float yrt_tile_error(const float* accu4, const float* half4, int width, int height, int tx, int ty) {
  float slots[YRT_TILE_ERROR_SLOTS];
  for (int k = 0; k < YRT_TILE_ERROR_SLOTS; ++k) {
    const int x = tx * 16 + (k & 15), y = ty * 16 + (k >> 4);
    const unsigned long long pix = (unsigned long long)y * (unsigned long long)width + (unsigned long long)x;
    slots[k] = x < width && y < height ? yrt_pixel_error(accu4 + pix * 4, half4 + pix * 4) : 0.0f;
  }
  for (int h = YRT_TILE_ERROR_SLOTS / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; ++i) yrt_tile_tree_step(slots, i, h);
  return yrt_tile_error_mean(slots[0], yrt_tile_pixels(tx, ty, width, height));
}
