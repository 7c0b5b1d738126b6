// yrt_pixel_variance.h — the per-pixel variance of a displayed frame, from the two accumulations an
// adaptive render keeps (device/adaptive.cpp): the running sums S (weight w, every iteration) and
// the half sums H (weight h, the even iterations). The odd iterations are S - H (weight r = w - h),
// so the frame is the weighted mean of two independent halves:
//   A_c  = H_c * rcp(h),  B_c = max(S_c - H_c, 0) * rcp(r)          (c = r, g, b; linear radiance)
//   dA_c = T(A_c),  dB_c = T(B_c)     T: the tone mapper's display mapping as k_resolve_pixels applies
//                                     it, pow(., 1 / gamma) iff gamma != 1, then the vignette iff set
//   f    = (h * r) * (rcp(w) * rcp(w))
//   v_c  = ((dA_c - dB_c) * (dA_c - dB_c)) * f
// (dA - dB)^2 estimates var(A) + var(B); the mean (h A + r B) / w of halves whose variances go as
// 1 / h and 1 / r has the variance h r / w^2 of that sum: f, 1/4 when the halves are equal.
// A v_c that is not finite (a half without samples, a non-finite sum) is stored as 0.
//
// Stated once for the device (k_frame_variance, kernels/k_denoise.h) and the host
// (yrtDebugFrameVariance). With gamma 1 and no vignette only + - * max and the reference's rcp
// (yrt_sse_rcp.h) are used, which give the same bits on both; T's pow and cos are yrt_libm.h's.
// Both sides are compiled without FMA contraction.
#pragma once

#include "yrt_libm.h"
#include "yrt_sse_rcp.h"

// DefaultToneMapper's vignette factor of pixel (x, y), as k_resolve_pixels computes it
YRT_SSE_FN float yrt_vignette_factor(int x, int y, int width, int height) {
  const float rw = yrt_ref_rcp(0.5f * (float)width);
  const float vx = ((float)x - 0.5f * (float)width) * rw, vy = ((float)y - 0.5f * (float)height) * rw;
  const float d = __builtin_sqrtf(vx * vx + vy * vy);
  return yrt_powf(yrt_cosf(d * 0.5f), 3.0f);
}

// one pixel: S = (sum.rgb, w), H = (half sum.rgb, h) -> var4 = (v_r, v_g, v_b, 1)
YRT_SSE_FN void yrt_pixel_variance(const float* S, const float* H, int x, int y, int width, int height, float gamma,
                                   float rcpGamma, int vignetting, float* var4) {
  const float h = H[3], r = S[3] - h;
  const float rh = yrt_ref_rcp(h), rr = yrt_ref_rcp(r), rw = yrt_ref_rcp(S[3]);
  const float f = (h * r) * (rw * rw);
  const float vig = vignetting ? yrt_vignette_factor(x, y, width, height) : 1.0f;
  for (int c = 0; c < 3; ++c) {
    float A = H[c] * rh, B = __builtin_fmaxf(S[c] - H[c], 0.0f) * rr;
    if (gamma != 1.0f) {
      A = yrt_powf(A, rcpGamma);
      B = yrt_powf(B, rcpGamma);
    }
    if (vignetting) {
      A = A * vig;
      B = B * vig;
    }
    const float d = A - B;
    const float v = (d * d) * f;
    var4[c] = (yrt_sse_bits(v) & 0x7f800000u) != 0x7f800000u ? v : 0.0f;
  }
  var4[3] = 1.0f;
}
