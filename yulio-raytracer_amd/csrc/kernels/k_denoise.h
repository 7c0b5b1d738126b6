// k_denoise.h — the denoiser's filter: the framebuffer load (with demodulation) and the
// edge-avoiding à-trous iterations; its guide frames come from k_guides (k_firsthit.h). The
// variance-guided kernels (k_frame_variance, k_atrous_load_var, k_atrous_var) share the bodies of
// the plain ones: VAR is a compile-time switch, the plain instantiations hold none of its code.
#pragma once

#include "yrt_kernels.h"
#include "yrt_wave.h"
#include "../common/yrt_cube_tap.h"
#include "../common/yrt_libm.h"
#include "../common/yrt_pixel_variance.h"

namespace yrt {

// A framebuffer as the filter reads and writes it: float or 8-bit channels, 3 or 4 per pixel,
// rows rowStride channels apart (RGB8 rows are padded to 4 bytes).
__device__ __forceinline__ size_t fb_channel(const FrameIO& io, int x, int y) {
  return (size_t)y * io.rowStride + (size_t)x * io.pixStride;
}

// c_0 of the filter: the framebuffer's pixels as float4 (8-bit channels as byte / 255), one
// width x height frame per face: blockIdx.y is the face, its pixels are those of faceIo[face] and
// dst, albedo4 and mod4 are [face][height][width] arrays.
// DEMOD (YRTDenoiseParams::demodulate): a hit pixel's modulation m = max(albedo, floor) ^ power
// per channel goes to mod4 and the filter's input is d_0 = c_0 / m (IEEE divisions); a miss
// pixel, which the filter neither reads nor writes, keeps c_0 and gets m = 1.
// VAR (k_atrous_load_var): dst.w, 0 in the plain filter, receives the pixel's scalar variance
// v_0 = v_r + v_g + v_b of var4 (k_frame_variance), with DEMOD sum_c v_c / m_c^2, the variance of
// the quotient; 0 on a miss (pos4.w = inf). It then rides in the 16 bytes every tap loads.
template <bool DEMOD, bool VAR>
__device__ __forceinline__ void atrous_load_body(const FrameIO* __restrict__ faceIo, int width, int height,
                                                 float4* __restrict__ dst, const float4* __restrict__ albedo4,
                                                 float albedoFloor, float albedoPower, float4* __restrict__ mod4,
                                                 const float4* __restrict__ var4, const float4* __restrict__ pos4) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)width * height) return;
  const int y = (int)(i / width), x = (int)(i - (long long)y * width);
  i += (long long)blockIdx.y * width * height;
  const FrameIO io = faceIo[blockIdx.y];
  const size_t o = fb_channel(io, x, y);
  float4 c;
  if (io.bytes) {
    const uint8_t* p = (const uint8_t*)io.pixels + o;
    c = make_float4(float(p[0]) / 255.0f, float(p[1]) / 255.0f, float(p[2]) / 255.0f, 0.f);
  } else {
    const float* p = (const float*)io.pixels + o;
    c = make_float4(p[0], p[1], p[2], 0.f);
  }
  float4 m = make_float4(1.f, 1.f, 1.f, 0.f);
  if constexpr (DEMOD) {
    const float4 a = albedo4[i];
    if (a.w != 0.f) {
      m.x = yrt_powf(fmaxf(a.x, albedoFloor), albedoPower);
      m.y = yrt_powf(fmaxf(a.y, albedoFloor), albedoPower);
      m.z = yrt_powf(fmaxf(a.z, albedoFloor), albedoPower);
      c = make_float4(c.x / m.x, c.y / m.y, c.z / m.z, 0.f);
    }
    mod4[i] = m;
  }
  if constexpr (VAR) {
    if (pos4[i].w < __int_as_float(0x7f800000)) {
      const float4 v = var4[i];
      c.w = DEMOD ? (v.x / (m.x * m.x) + v.y / (m.y * m.y)) + v.z / (m.z * m.z) : (v.x + v.y) + v.z;
    }
  }
  dst[i] = c;
}

template <bool DEMOD>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous_load(const FrameIO* __restrict__ faceIo, int width, int height,
                                                           float4* __restrict__ dst,
                                                           const float4* __restrict__ albedo4, float albedoFloor,
                                                           float albedoPower, float4* __restrict__ mod4) {
  atrous_load_body<DEMOD, false>(faceIo, width, height, dst, albedo4, albedoFloor, albedoPower, mod4, nullptr, nullptr);
}

template <bool DEMOD>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous_load_var(const FrameIO* __restrict__ faceIo, int width,
                                                               int height, float4* __restrict__ dst,
                                                               const float4* __restrict__ albedo4, float albedoFloor,
                                                               float albedoPower, float4* __restrict__ mod4,
                                                               const float4* __restrict__ var4,
                                                               const float4* __restrict__ pos4) {
  atrous_load_body<DEMOD, true>(faceIo, width, height, dst, albedo4, albedoFloor, albedoPower, mod4, var4, pos4);
}

// The variance frame of one face (yrt_pixel_variance.h): var4 = (v_r, v_g, v_b, 1) of the displayed
// frame from the framebuffer's sums and half sums, one thread per pixel.
__global__ __launch_bounds__(YRT_BLOCK) void k_frame_variance(const float4* __restrict__ accu,
                                                              const float4* __restrict__ half, int width, int height,
                                                              float gamma, float rcpGamma, int vignetting,
                                                              float4* __restrict__ var4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)width * height) return;
  const int y = (int)(i / width), x = (int)(i - (long long)y * width);
  const float4 S = accu[i], H = half[i];
  const float s4[4] = {S.x, S.y, S.z, S.w}, h4[4] = {H.x, H.y, H.z, H.w};
  float v[4];
  yrt_pixel_variance(s4, h4, x, y, width, height, gamma, rcpGamma, vignetting, v);
  var4[i] = make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ float atrous_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One iteration of the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) with
// SVGF's normal and plane-distance weights: 5x5 taps `step` pixels apart, the
// B3-spline kernel h = (1/16, 1/4, 3/8, 1/4, 1/16) per axis, times
//   w_n = max(0, n_p . n_q) ^ sigmaNormal
//   w_x = exp(-|n_p . (x_q - x_p)| / (sigmaPosition t_p))
//   w_c = exp(-|c_p - c_q|^2 / sigmaColor_i^2)                  (rcpSigmaColor2 = 0: off)
// Taps on a miss are skipped; the centre tap weighs h(0)^2 exactly. The mean is taken as
// c_p + sum w (c_q - c_p) / sum w, so a constant frame stays what it is. A miss pixel is not
// written. The frames are [face][height][width] arrays and blockIdx.y is the face. A tap that
// leaves its face is skipped, or, with WRAP (yrtDenoiseCube: square faces, six per eye in
// cubeFaceIndex order), reads the pixel yrt_cube_tap names on a neighbour of the same eye (a
// corner tap is skipped), with the same weights. The last iteration (faceOut != null) stores face
// f's pixels into the framebuffer faceOut[f]: floats as they are, bytes as k_resolve_pixels
// quantizes them; alpha and row padding are not touched. DEMOD: the frames hold the demodulated
// signal d (k_atrous_load), every weight acts on d, and the last iteration stores d_n m with the
// modulation of mod4.
//
// VAR (k_atrous_var, the variance-guided filter after SVGF, Schied et al. 2017): src.w holds the
// scalar variance v_i of the pixel's colour, and the colour weight's width is the local standard
// deviation instead of sigmaColor_i:
//   vbar_p = sum g v_i(q) / sum g over the 3x3 neighbours one pixel (not one step) apart,
//            g = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), skipping taps off the surface or on a miss
//   w_c    = exp(-|c_p - c_q|^2 / (sigmaVariance^2 vbar_p + varianceFloor))
//   v_i+1  = sum w^2 v_i(q) / (sum w)^2, the centre with w = h(0)^2, stored in dst.w
// The eight neighbours cost two 4-byte loads each (hit or miss, v_i) beside the lanes' own pixels.
template <bool DEMOD, bool WRAP, bool VAR>
__device__ __forceinline__ void atrous_body(const AtrousParams& ap, const float4* __restrict__ pos4,
                                            const float4* __restrict__ nrm4, const float4* __restrict__ src,
                                            float4* __restrict__ dst, const float4* __restrict__ mod4,
                                            const FrameIO* __restrict__ faceOut, float sigmaVariance2,
                                            float varianceFloor) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ap.width * ap.height) return;
  const int y = (int)(i / ap.width), x = (int)(i - (long long)y * ap.width);
  const int face = (int)blockIdx.y;
  const size_t base = (size_t)face * ap.width * ap.height;  // of this face's frame
  i += (long long)base;
  const float INF = __int_as_float(0x7f800000);
  const float4 pp = pos4[i];
  if (!(pp.w < INF)) return;
  const float4 n4 = nrm4[i], c4 = src[i];
  const V3 xp = v3(pp.x, pp.y, pp.z), np = v3(n4.x, n4.y, n4.z), cp = v3(c4.x, c4.y, c4.z);
  const float rcpPlane = 1.0f / (ap.sigmaPosition * pp.w);
  V3 sum = v3s(0.f);
  float wsum = atrous_h(0) * atrous_h(0);
  float rcpVariance = 0.f, vsum = 0.f;
  if constexpr (VAR) {
    float gv = 0.25f * c4.w, gsum = 0.25f;
    for (int ey = -1; ey <= 1; ++ey)
      for (int ex = -1; ex <= 1; ++ex) {
        if (ex == 0 && ey == 0) continue;
        size_t j;
        if constexpr (WRAP) {
          int g, tx, ty;
          if (yrt_cube_tap(ap.width, face % 6, x + ex, y + ey, &g, &tx, &ty) != 1) continue;
          j = ((size_t)(face - face % 6 + g) * ap.height + (size_t)ty) * ap.width + (size_t)tx;
        } else {
          if (x + ex < 0 || x + ex >= ap.width || y + ey < 0 || y + ey >= ap.height) continue;
          j = base + (size_t)(y + ey) * ap.width + (size_t)(x + ex);
        }
        if (!(pos4[j].w < INF)) continue;
        const float g = (ex == 0 ? 0.5f : 0.25f) * (ey == 0 ? 0.5f : 0.25f);
        gv = gv + g * src[j].w;
        gsum = gsum + g;
      }
    rcpVariance = 1.0f / (sigmaVariance2 * (gv / gsum) + varianceFloor);
    vsum = (wsum * wsum) * c4.w;
  }
  for (int dy = -2; dy <= 2; ++dy) {
    const long long qy = (long long)y + (long long)dy * ap.step;
    if (!WRAP && (qy < 0 || qy >= ap.height)) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const long long qx = (long long)x + (long long)dx * ap.step;
      size_t j;
      if constexpr (WRAP) {
        if (dx == 0 && dy == 0) continue;
        int g, tx, ty;  // the host keeps W and the step inside yrt_cube_tap's range
        if (yrt_cube_tap(ap.width, face % 6, (int)qx, (int)qy, &g, &tx, &ty) != 1) continue;
        j = ((size_t)(face - face % 6 + g) * ap.height + (size_t)ty) * ap.width + (size_t)tx;
      } else {
        if (qx < 0 || qx >= ap.width || (dx == 0 && dy == 0)) continue;
        j = base + (size_t)qy * ap.width + (size_t)qx;
      }
      const float4 pq = pos4[j];
      if (!(pq.w < INF)) continue;
      const float4 nq = nrm4[j], cq4 = src[j];
      const V3 d = v3(cq4.x, cq4.y, cq4.z) - cp;
      float w = atrous_h(dx) * atrous_h(dy);
      w = w * yrt_powf(fmaxf(0.f, dot(np, v3(nq.x, nq.y, nq.z))), ap.sigmaNormal);
      w = w * yrt_expf(-fabsf(dot(np, v3(pq.x, pq.y, pq.z) - xp)) * rcpPlane);
      if constexpr (VAR) {
        w = w * yrt_expf(-dot(d, d) * rcpVariance);
        vsum = vsum + (w * w) * cq4.w;
      } else {
        if (ap.rcpSigmaColor2 > 0.f) w = w * yrt_expf(-dot(d, d) * ap.rcpSigmaColor2);
      }
      sum = sum + w * d;
      wsum = wsum + w;
    }
  }
  V3 c = cp + sum * (1.0f / wsum);
  if (!faceOut) {
    dst[i] = make_float4(c.x, c.y, c.z, VAR ? vsum / (wsum * wsum) : 0.f);
    return;
  }
  if constexpr (DEMOD) {
    const float4 m = mod4[i];
    c = c * v3(m.x, m.y, m.z);
  }
  const FrameIO out = faceOut[face];
  const size_t o = fb_channel(out, x, y);
  if (out.bytes) {
    uint8_t* p = (uint8_t*)out.pixels + o;
    p[0] = (uint8_t)clampf(c.x * 255.0f, 0.0f, 255.0f);
    p[1] = (uint8_t)clampf(c.y * 255.0f, 0.0f, 255.0f);
    p[2] = (uint8_t)clampf(c.z * 255.0f, 0.0f, 255.0f);
  } else {
    float* p = (float*)out.pixels + o;
    p[0] = c.x;
    p[1] = c.y;
    p[2] = c.z;
  }
}

template <bool DEMOD, bool WRAP>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous(AtrousParams ap, const float4* __restrict__ pos4,
                                                      const float4* __restrict__ nrm4, const float4* __restrict__ src,
                                                      float4* __restrict__ dst, const float4* __restrict__ mod4,
                                                      const FrameIO* __restrict__ faceOut) {
  atrous_body<DEMOD, WRAP, false>(ap, pos4, nrm4, src, dst, mod4, faceOut, 0.f, 0.f);
}

template <bool DEMOD, bool WRAP>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous_var(AtrousParams ap, const float4* __restrict__ pos4,
                                                          const float4* __restrict__ nrm4,
                                                          const float4* __restrict__ src, float4* __restrict__ dst,
                                                          const float4* __restrict__ mod4,
                                                          const FrameIO* __restrict__ faceOut, float sigmaVariance2,
                                                          float varianceFloor) {
  atrous_body<DEMOD, WRAP, true>(ap, pos4, nrm4, src, dst, mod4, faceOut, sigmaVariance2, varianceFloor);
}

}  // namespace yrt
