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

// ---------------------------------------------------------------- material probe
// k_check_material<MM> (yrtDebugMaterial mode 0, test-only): Material::shade of one geometry of a
// committed scene as k_shade<MM> performs it, one thread per row: the geometry's record through
// geom_burst<MM>, shade_material<MM> on the row's dg, then comp_eval and comp_sample of every
// component it created (after shade_material: Obj's bump map has turned dg.Ns by then). It holds
// no formula of its own; the pieces of the record that MM's burst leaves out stay zero, as in
// k_shade.
//   rows  n x 22 words: wo, Ns, Ng, Tx, Ty, wi (3 each), s.xy, then dg.s, dg.t
//   out   n x 34 words: the component count, then 3 x (comp_type(kind), eval3, sample3, wi3, pdf),
//         zero beyond the count (oracle/ref_shade.cpp's ref_material_components)
// medium: the current medium's index in the scene's medium table.
#define YRT_MAT_ROW 22
#define YRT_MAT_OUT 34
template <unsigned MM>
__global__ __launch_bounds__(64) void k_check_material(SceneView sv, int geom, int medium, int n,
                                                       const float* __restrict__ rows, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr unsigned CM = comps_of(MM);
  const float* r = rows + (size_t)i * YRT_MAT_ROW;
  float* o = out + (size_t)i * YRT_MAT_OUT;
  GeomHead gh;
  GpuMaterial gm = {};
  GpuTexture gt0 = {};
  geom_burst<MM>(sv.geomRecs + geom, gh, gm, gt0);
  const V3 wo = v3(r[0], r[1], r[2]), wi = v3(r[15], r[16], r[17]);
  DG dg;
  dg.P = v3s(0.f);
  dg.Ns = v3(r[3], r[4], r[5]);
  dg.Ng = v3(r[6], r[7], r[8]);
  dg.Tx = v3(r[9], r[10], r[11]);
  dg.Ty = v3(r[12], r[13], r[14]);
  dg.s = r[20];
  dg.t = r[21];
  dg.error = 0.f;
  dg.material = gh.material;
  dg.light = -1;
  dg.illumMask = dg.shadowMask = -1;
  BRDFSet bs;
  bs.n = 0;
#pragma unroll
  for (int k = 0; k < YRT_MAX_COMPS; ++k) {
    bs.c[k].kind = 0;
    bs.c[k].R = v3s(0.f);
    bs.c[k].a = bs.c[k].b = bs.c[k].c = 0.f;
  }
  if (dg.material >= 0) shade_material<MM>(sv, gm, gt0, dg.material, medium, dg, bs);
  dg_frame(dg);
  const float4 sd = sample_dir(r[18], r[19]);
  o[0] = __int_as_float(bs.n);
#pragma unroll
  for (int k = 0; k < YRT_MAX_COMPS; ++k) {
    float* c = o + 1 + 11 * k;
    V3 e = v3s(0.f), sa = v3s(0.f), w = v3s(0.f);
    float pdf = 0.f;
    uint32_t type = 0;
    if (k < bs.n) {
      type = comp_type(bs.c[k].kind);
      e = comp_eval<CM>(bs.c[k], sv.materials, wo, dg, wi);
      sa = comp_sample<CM>(bs.c[k], sv.materials, wo, dg, sd, r[19], w, pdf);
    }
    c[0] = __uint_as_float(type);
    c[1] = e.x; c[2] = e.y; c[3] = e.z;
    c[4] = sa.x; c[5] = sa.y; c[6] = sa.z;
    c[7] = w.x; c[8] = w.y; c[9] = w.z;
    c[10] = pdf;
  }
}

// k_check_textures (yrtDebugMaterial mode 1, test-only): the texture lookups of one geometry's
// material at raw (s, t), one thread per row; the material's s0 / ds are not applied.
//   st   n x 2 words
//   out  n x 24 words: RGBA of tex_get(m.tex[k]) for k = 0..4 (zero where m.tex[k] < 0), then RGBA of
//        tex_get_rec over the descriptor copy GpuGeomRec::t0 as geom_burst hands it to k_shade
//        (zero where m.tex[0] < 0)
#define YRT_TEX_OUT 24
__global__ __launch_bounds__(64) void k_check_textures(SceneView sv, int geom, int n, const float* __restrict__ st,
                                                       float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = st[2 * i], t = st[2 * i + 1];
  float* o = out + (size_t)i * YRT_TEX_OUT;
  GeomHead gh;
  GpuMaterial gm = {};
  GpuTexture gt0 = {};
  geom_burst<YRT_ALL_MATS>(sv.geomRecs + geom, gh, gm, gt0);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < 5) {
      if (gm.tex[k] >= 0) tex_get(sv.textures, sv.images, sv.texels, sv.texQuads, gm.tex[k], s, t, c);
    } else if (gm.tex[0] >= 0) {
      tex_get_rec(gt0, sv.texels, sv.texQuads, s, t, c);
    }
    o[4 * k] = c[0]; o[4 * k + 1] = c[1]; o[4 * k + 2] = c[2]; o[4 * k + 3] = c[3];
  }
}

}  // namespace yrt
