// k_checks.h — test-only self-checks: the arithmetic checks over every 32-bit pattern and the
// shading-layer probe.
#pragma once

#include "yrt_camera.h"
#include "yrt_shade.h"
#include "yrt_surface.h"
#include "../common/yrt_sse_rcp.h"

namespace yrt {

// ---------------------------------------------------------------- arithmetic checks
// fn 0: rcp_rn(x) against the IEEE division 1.0f/x for every 32-bit pattern x.
// Mismatches are counted in out[0]; out[1] = the smallest mismatching input bits.
__global__ __launch_bounds__(256) void k_check_math(int fn, unsigned long long* out) {
  unsigned long long bad = 0, first = ~0ull;
  if (fn == 0) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < (1ull << 32);
         i += (unsigned long long)gridDim.x * 256ull) {
      const float x = __uint_as_float((uint32_t)i);
      const float got = rcp_rn(x), want = 1.0f / x;
      if (!(__float_as_uint(got) == __float_as_uint(want) || (got != got && want != want))) {
        ++bad;
        first = i < first ? i : first;
      }
    }
  }
  if (bad) {
    atomicAdd(&out[0], bad);
    atomicMin(&out[1], first);
  }
}

// fn 1 / 2: the emulated SSE estimates yrt_rcpps / yrt_rsqrtps (common/yrt_sse_rcp.h) against a
// reconstruction from the 2048-entry table `tab` of 12-bit mantissas (the Intel fixture,
// tests/golden/sse_rcp_tables.json), for every 32-bit pattern; written independently of the
// emulation (the reconstruction of tests/test_sse_rcp.py).
__device__ __forceinline__ uint32_t sse_expect(int fn, uint32_t u, const uint16_t* tab) {
  const uint32_t s = u >> 31, e = (u >> 23) & 0xffu, mant = u & 0x7fffffu;
  if (fn == 1) {
    if (e == 0u) return (s << 31) | 0x7f800000u;
    if (e == 255u) return mant ? (u | 0x400000u) : (s << 31);
    if (e >= 253u) return s << 31;
    return (s << 31) | ((253u - e) << 23) | ((uint32_t)tab[(u >> 12) & 0x7ffu] << 11);
  }
  if (e == 0u) return (s << 31) | 0x7f800000u;
  if (e == 255u && mant) return u | 0x400000u;
  if (s) return 0xffc00000u;
  if (e == 255u) return 0u;
  const int E = (int)e - 127, p = E & 1, k = (E - p) / 2;
  return ((uint32_t)(126 - k) << 23) | ((uint32_t)tab[((uint32_t)p << 10) | ((u >> 13) & 0x3ffu)] << 11);
}
__global__ __launch_bounds__(256) void k_check_math_table(int fn, const uint16_t* __restrict__ tab,
                                                          unsigned long long* out) {
  unsigned long long bad = 0, first = ~0ull;
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < (1ull << 32);
       i += (unsigned long long)gridDim.x * 256ull) {
    const uint32_t u = (uint32_t)i;
    const float x = __uint_as_float(u);
    const uint32_t got = __float_as_uint(fn == 1 ? yrt_rcpps(x) : yrt_rsqrtps(x));
    if (got != sse_expect(fn, u, tab)) {
      ++bad;
      first = i < first ? i : first;
    }
  }
  if (bad) {
    atomicAdd(&out[0], bad);
    atomicMin(&out[1], first);
  }
}

// fn 3 / 4: yrt_rcpps / yrt_rsqrtps of n given inputs, bits in and bits out in place (the special
// inputs of tests/test_sse_rcp_special.py against the host's emulation)
__global__ __launch_bounds__(256) void k_check_math_values(int fn, int n, unsigned long long* io) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float((uint32_t)io[i]);
  io[i] = __float_as_uint(fn == 3 ? yrt_rcpps(x) : yrt_rsqrtps(x));
}

// ---------------------------------------------------------------- shading-layer probe
// k_check_shade (yrtDebugShade, test-only): one thread per row calls the device functions of the
// shading layer as they stand, so that their results can be compared bit for bit with the
// reference's own classes (tests/test_ref_shade.py). It holds no formula of its own.
//   rows  n x 48 words: wo, Ns, Ng, Tx, Ty, wi (3 each), s.xy, ss, the component count, 2 pad,
//         then 3 components of 8 words: kind, R.rgb, a, b, c, pad (conductor kinds: c = the
//         index of their record in mats, as Material::shade stores it)
//   out   n x 12 words
//   mode 0  comp_eval at wi and comp_sample at s of component 0: eval, sample, wi (3 each), pdf
//   mode 1  set_sample of the components at (s, ss): colour, wi (3 each), pdf, type bits
//   mode 2  camera_ray of *cam at pixel = wo.xy, lens = s: org, dir
//   mode 3  light_sample of *light at P = wo on the frame Ns, with s: L, wi (3 each), pdf
// Every-material component mask and every light type, as k_shade's widest instantiation. Off
// the render loop: its state may live in scratch.
#define YRT_SHADE_ROW 48
#define YRT_SHADE_OUT 12
__global__ __launch_bounds__(64) void k_check_shade(int mode, int n, const float* __restrict__ rows,
                                                    const GpuMaterial* __restrict__ mats,
                                                    const GpuCamera* __restrict__ cam,
                                                    const GpuLight* __restrict__ light, float* __restrict__ out) {
  __shared__ float st[21 * 64];  // set_sample's candidate slots, [21][64]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr unsigned CM = comps_of(YRT_ALL_MATS);
  const float* r = rows + (size_t)i * YRT_SHADE_ROW;
  float* o = out + (size_t)i * YRT_SHADE_OUT;
  const V3 wo = v3(r[0], r[1], r[2]), wi = v3(r[15], r[16], r[17]);
  DG dg;
  dg.P = wo;  // mode 3 only
  dg.Ns = v3(r[3], r[4], r[5]);
  dg.Ng = v3(r[6], r[7], r[8]);
  dg.Tx = v3(r[9], r[10], r[11]);
  dg.Ty = v3(r[12], r[13], r[14]);
  dg.s = dg.t = dg.error = 0.f;
  dg.material = dg.light = -1;
  dg.illumMask = dg.shadowMask = -1;
  dg_frame(dg);
  const float sx = r[18], sy = r[19], ss = r[20];
  const float4 sd = sample_dir(sx, sy);  // as k_sample_dirs tabulates it for k_shade
  BRDFSet bs;
  bs.n = __float_as_int(r[21]);
#pragma unroll
  for (int k = 0; k < YRT_MAX_COMPS; ++k) {
    const float* c = r + 24 + 8 * k;
    bs.c[k].kind = __float_as_int(c[0]);
    bs.c[k].R = v3(c[1], c[2], c[3]);
    bs.c[k].a = c[4];
    bs.c[k].b = c[5];
    bs.c[k].c = c[6];
  }
  V3 a = v3s(0.f), b = v3s(0.f), w = v3s(0.f);
  float pdf = 0.f;
  if (mode == 0) {
    a = comp_eval<CM>(bs.c[0], mats, wo, dg, wi);
    b = comp_sample<CM>(bs.c[0], mats, wo, dg, sd, sy, w, pdf);
    o[9] = pdf;
    o[10] = o[11] = 0.f;
  } else if (mode == 1) {
    uint32_t type = 0;
    a = set_sample<CM>(bs, mats, wo, dg, sd, sy, ss, b, pdf, type, st + threadIdx.x);
    o[6] = pdf;
    o[7] = __uint_as_float(type);
    o[8] = o[9] = o[10] = o[11] = 0.f;
  } else if (mode == 2) {
    camera_ray(*cam, r[0], r[1], a, b, sx, sy);
  } else {
    a = light_sample<kAllLights>(*light, dg, sd, sx, sy, b, pdf);
    o[6] = pdf;
    o[7] = o[8] = o[9] = o[10] = o[11] = 0.f;
  }
  o[0] = a.x; o[1] = a.y; o[2] = a.z;
  o[3] = b.x; o[4] = b.y; o[5] = b.z;
  if (mode == 0) { o[6] = w.x; o[7] = w.y; o[8] = w.z; }
  if (mode == 2) o[6] = o[7] = o[8] = o[9] = o[10] = o[11] = 0.f;
}

}  // namespace yrt
