// k_aux.h — the kernels off the render loop: the debug renderer, rtPick, the multi-GPU tile
// slabs, the arithmetic self-checks, and the BVH refit and node quantization.
#pragma once

#include "yrt_camera.h"
#include "yrt_shade.h"
#include "yrt_surface.h"
#include "yrt_traverse.h"

namespace yrt {

// DebugRenderer (renderers/debugrenderer.cpp:66-140): one thread per 16x16 tile, since the
// per-tile Random is consumed sequentially in scan order.
__global__ __launch_bounds__(64) void k_debug(SceneView sv, FrameView fv, int maxDepth, int spp,
                                             float* __restrict__ fbFloat, uint8_t* __restrict__ fbRGB8,
                                             int rgb8Stride) {
  __shared__ int stack[YRT_LDS_STACK * YRT_TRACE_BLOCK];
  const GpuRenderParams& rp = *fv.rp;
  const GpuCamera& cam = *fv.cam;
  const int tile = blockIdx.x * blockDim.x + threadIdx.x;
  if (tile >= rp.numTilesX * rp.numTilesY) return;
  DevRandom rnd;
  rnd.setSeed(tile * 1024);
  const int x0 = (tile % rp.numTilesX) * 16, y0 = (tile / rp.numTilesX) * 16;
  for (int dy = 0; dy < 16; dy++) {
    const int iy = y0 + dy;
    const float fy = iy * rp.rcpHeight;
    if (iy >= rp.height) continue;
    for (int dx = 0; dx < 16; dx++) {
      const int ix = x0 + dx;
      const float fx = ix * rp.rcpWidth;
      if (ix >= rp.width) continue;
      for (int i = 0; i < spp; i++) {
        V3 org, dir;
        camera_ray(cam, fx, fy, org, dir);
        float tnear = 0.f, tfar = __int_as_float(0x7f800000);
        Hit h;
        h.tri = -1;
        int id0 = -1, id1 = -1;
        for (int depth = 0; depth < maxDepth; depth++) {
          RayPre r;
          r.org = org;
          r.dir = dir;
          r.inv = v3(safe_inv(dir.x), safe_inv(dir.y), safe_inv(dir.z));
          r.tnear = tnear;
          r.tfar = tfar;
          h = traverse<false>(sv.nodes, sv.tris, r, stack + threadIdx.x);
          if (h.tri < 0) {
            id0 = id1 = -1;
            break;
          }
          const int g = sv.triGeom[h.tri];
          id0 = g;
          id1 = h.tri - sv.geoms[g].triBase;
          if (depth + 1 < maxDepth) {
            const int4 idx = sv.indices[h.tri];
            const V3 p0 = ld3(sv.positions[idx.x]), p1 = ld3(sv.positions[idx.y]), p2 = ld3(sv.positions[idx.z]);
            const V3 Ng = cross(p0 - p1, p2 - p0);  // ray.Ng
            V3 Nf = normalize(Ng);
            if (dot(-dir, Nf) < 0) Nf = -Nf;
            const float u1 = rnd.getFloat();
            const float u2 = rnd.getFloat();
            float pdf;
            const V3 norg = org + 0.999f * h.t * dir;
            dir = cosine_hemi(u1, u2, Nf, pdf);
            org = norg;
            tnear = 4.0f * kUlp;
            tfar = __int_as_float(0x7f800000);
          }
        }
        V3 c;
        if (id0 < 0) c = v3s(1.0f);
        else
          c = v3(((3434553u * ((unsigned)(id0 + id1 + 3243))) % 255) / 255.0f,
                 ((7342453u * ((unsigned)(id0 + id1 + 8237))) % 255) / 255.0f,
                 ((9234454u * ((unsigned)(id0 + id1 + 2343))) % 255) / 255.0f);
        if (fbFloat) {
          float* o = fbFloat + ((size_t)iy * rp.width + ix) * 3;
          o[0] = c.x;
          o[1] = c.y;
          o[2] = c.z;
        }
        if (fbRGB8) {
          uint8_t* o = fbRGB8 + (size_t)iy * rgb8Stride + 3 * ix;
          o[0] = (uint8_t)clampf(c.x * 255.0f, 0.0f, 255.0f);
          o[1] = (uint8_t)clampf(c.y * 255.0f, 0.0f, 255.0f);
          o[2] = (uint8_t)clampf(c.z * 255.0f, 0.0f, 255.0f);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- multi-GPU tile slabs
// Slab pixel i of a shard's tile sequence -> (frame f, x, y); frames are numFrames images of
// width x height stacked in memory, tile t = frame t / tilesPerFrame.
__device__ __forceinline__ bool slab_pixel(const SlabLayout& L, int i, int& f, int& x, int& y) {
  const int ntx = (L.width + 15) >> 4;
  int t = L.tileOffset + (i >> 8) * L.tileStride;
  f = t / L.tilesPerFrame;
  t -= f * L.tilesPerFrame;
  if (L.tileStride > 1) t = yrt_tile_scatter(t, L.tilesPerFrame);  // as batch_tile
  x = (t % ntx) * 16 + (i & 15);
  y = (t / ntx) * 16 + ((i >> 4) & 15);
  return x < L.width && y < L.height;
}

// rgb8: the slab holds one 32-bit word per pixel (the RGB8 bytes, what an RGB8 framebuffer
// maps); else float4 (the float pixel, w = the RGB8 bytes)
__global__ __launch_bounds__(256) void k_pack_tiles(const float* __restrict__ fbFloat,
                                                    const uint8_t* __restrict__ fbRGB8, SlabLayout L, int n,
                                                    void* __restrict__ slab) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int f, x, y;
    const bool in = slab_pixel(L, i, f, x, y);
    unsigned c = 0;
    if (in) {
      const uint8_t* p = fbRGB8 + ((size_t)f * L.height + y) * L.rgb8Stride + 3 * x;
      c = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
    if (L.rgb8) {
      ((unsigned*)slab)[i] = c;
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, __uint_as_float(c));
      if (in) {
        const float* fp = fbFloat + (((size_t)f * L.height + y) * L.width + x) * 3;
        v.x = fp[0];
        v.y = fp[1];
        v.z = fp[2];
      }
      ((float4*)slab)[i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_unpack_tiles(const void* __restrict__ slab, float* __restrict__ fbFloat,
                                                      uint8_t* __restrict__ fbRGB8, SlabLayout L, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int f, x, y;
    if (!slab_pixel(L, i, f, x, y)) continue;
    unsigned c;
    if (L.rgb8) {
      c = ((const unsigned*)slab)[i];
    } else {
      const float4 v = ((const float4*)slab)[i];
      float* fp = fbFloat + (((size_t)f * L.height + y) * L.width + x) * 3;
      fp[0] = v.x;
      fp[1] = v.y;
      fp[2] = v.z;
      c = __float_as_uint(v.w);
    }
    uint8_t* o = fbRGB8 + ((size_t)f * L.height + y) * L.rgb8Stride + 3 * x;
    o[0] = (uint8_t)(c & 255u);
    o[1] = (uint8_t)((c >> 8) & 255u);
    o[2] = (uint8_t)((c >> 16) & 255u);
  }
}

// SingleRayDevice::rtPick (api/singleray_device.cpp:692-708): one camera ray at image-plane
// (x, y), lens sample (0.5, 0.5), closest hit.
__global__ __launch_bounds__(YRT_TRACE_BLOCK) void k_pick(SceneView sv, const GpuCamera* camp, float x, float y,
                                                          float4* out) {
  __shared__ int stack[YRT_LDS_STACK * YRT_TRACE_BLOCK];
  if (threadIdx.x != 0) return;
  V3 org, dir;
  camera_ray(*camp, x, y, org, dir);
  RayPre r;
  r.org = org;
  r.dir = dir;
  r.inv = v3(safe_inv(dir.x), safe_inv(dir.y), safe_inv(dir.z));
  r.tnear = 0.f;
  r.tfar = __int_as_float(0x7f800000);
  const Hit h = traverse<false>(sv.nodes, sv.tris, r, stack + threadIdx.x);
  const V3 p = org + h.t * dir;
  out[0] = make_float4(p.x, p.y, p.z, __int_as_float(h.tri));
}

// ---------------------------------------------------------------- denoise: guides + filter
// First-hit guide buffers (yrtRenderGuides, the denoiser's input): pixel (x, y) traces k_pick's
// ray through the image-plane point ((x + .5) / W, (y + .5) / H) (IEEE divisions: the float a
// caller computes for rtPick), time 0, and stores pos4 = (org + t dir, t) and nrm4 = (Ns, 1)
// with postIntersect's shading normal turned towards the viewer; a miss stores (0, 0, 0, inf)
// and 0.
// ALBEDO (yrtRenderAlbedo, the demodulated filter): the same ray and hit also store
// albedo4 = (first-hit albedo, 1), a miss +0: Material::shade of the hit's material, evaluated
// on a copy of the differential geometry (Obj's bump map turns dg.Ns; the normal guide keeps
// postIntersect's) in the medium a camera ray starts in (vacuum, k_shade's depth 0), with
// k_shade's every-material instantiation and its tex_get / tex_get_rec. The albedo is the sum
// of R over the diffuse-reflection components; (1, 1, 1) where there is none, where the sum is
// 0 and on a light primitive. Off the render loop: its component set may live
// in scratch.
template <bool ALBEDO>
__global__ __launch_bounds__(YRT_TRACE_BLOCK) void k_guides(SceneView sv, const GpuCamera* camp, int width, int height,
                                                            float4* __restrict__ pos4, float4* __restrict__ nrm4,
                                                            float4* __restrict__ albedo4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)width * height) return;
  const int y = (int)(i / width), x = (int)(i - (long long)y * width);
  V3 org, dir;
  camera_ray(*camp, (float(x) + 0.5f) / float(width), (float(y) + 0.5f) / float(height), org, dir);
  RayPre r;
  r.org = org;
  r.dir = dir;
  r.inv = v3(safe_inv(dir.x), safe_inv(dir.y), safe_inv(dir.z));
  r.tnear = 0.f;
  r.tfar = __int_as_float(0x7f800000);
  const Hit h = traverse<false>(sv.nodes, sv.tris, r, nullptr);
  if (h.tri < 0) {
    pos4[i] = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7f800000));
    nrm4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (ALBEDO) albedo4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  DG dg;
  const int g = sv.triGeom[h.tri];
  post_intersect_g(sv, sv.geoms[g], org, dir, h.t, h.u, h.v, h.tri, dg, false);
  V3 n = dg.Ns;
  if (dot(n, dir) > 0.f) n = -n;
  pos4[i] = make_float4(dg.P.x, dg.P.y, dg.P.z, h.t);
  nrm4[i] = make_float4(n.x, n.y, n.z, 1.f);
  if constexpr (ALBEDO) {
    V3 a = v3s(0.f);
    if (dg.light < 0 && dg.material >= 0) {
      DG sdg = dg;  // shade_material may turn its Ns
      if (dot(sdg.Ng, dir) > 0.f) {  // k_shade hands Material::shade the viewer-facing side
        sdg.Ng = -sdg.Ng;
        sdg.Ns = -sdg.Ns;
      }
      BRDFSet bs;
      const GpuGeomRec& gr = sv.geomRecs[g];
      shade_material<YRT_ALL_MATS>(sv, gr.m, gr.t0, sdg.material, 0, sdg, bs);
#pragma unroll
      for (int k = 0; k < YRT_MAX_COMPS; ++k)
        if (k < bs.n && comp_type(bs.c[k].kind) == BT_DIFFUSE_REFLECTION) a = a + bs.c[k].R;
    }
    if (a == v3s(0.f)) a = v3s(1.f);
    albedo4[i] = make_float4(a.x, a.y, a.z, 1.f);
  }
}

// A framebuffer as the filter reads and writes it: float or 8-bit channels, 3 or 4 per pixel,
// rows rowStride channels apart (RGB8 rows are padded to 4 bytes).
__device__ __forceinline__ size_t fb_channel(const FrameIO& io, int x, int y) {
  return (size_t)y * io.rowStride + (size_t)x * io.pixStride;
}

// c_0 of the filter: the framebuffer's pixels as float4 (8-bit channels as byte / 255).
// DEMOD (YRTDenoiseParams::demodulate): a hit pixel's modulation m = max(albedo, floor) ^ power
// per channel goes to mod4 and the filter's input is d_0 = c_0 / m (IEEE divisions); a miss
// pixel, which the filter neither reads nor writes, keeps c_0 and gets m = 1.
template <bool DEMOD>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous_load(FrameIO io, float4* __restrict__ dst,
                                                           const float4* __restrict__ albedo4, float albedoFloor,
                                                           float albedoPower, float4* __restrict__ mod4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)io.width * io.height) return;
  const int y = (int)(i / io.width), x = (int)(i - (long long)y * io.width);
  const size_t o = fb_channel(io, x, y);
  float4 c;
  if (io.bytes) {
    const uint8_t* p = (const uint8_t*)io.pixels + o;
    c = make_float4(float(p[0]) / 255.0f, float(p[1]) / 255.0f, float(p[2]) / 255.0f, 0.f);
  } else {
    const float* p = (const float*)io.pixels + o;
    c = make_float4(p[0], p[1], p[2], 0.f);
  }
  if constexpr (DEMOD) {
    const float4 a = albedo4[i];
    float4 m = make_float4(1.f, 1.f, 1.f, 0.f);
    if (a.w != 0.f) {
      m.x = yrt_powf(fmaxf(a.x, albedoFloor), albedoPower);
      m.y = yrt_powf(fmaxf(a.y, albedoFloor), albedoPower);
      m.z = yrt_powf(fmaxf(a.z, albedoFloor), albedoPower);
      c = make_float4(c.x / m.x, c.y / m.y, c.z / m.z, 0.f);
    }
    mod4[i] = m;
  }
  dst[i] = c;
}

__device__ __forceinline__ float atrous_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One iteration of the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) with
// SVGF's normal and plane-distance weights: 5x5 taps `step` pixels apart, the
// B3-spline kernel h = (1/16, 1/4, 3/8, 1/4, 1/16) per axis, times
//   w_n = max(0, n_p . n_q) ^ sigmaNormal
//   w_x = exp(-|n_p . (x_q - x_p)| / (sigmaPosition t_p))
//   w_c = exp(-|c_p - c_q|^2 / sigmaColor_i^2)                  (rcpSigmaColor2 = 0: off)
// Taps outside the image or on a miss are skipped; the centre tap weighs h(0)^2 exactly. The
// mean is taken as c_p + sum w (c_q - c_p) / sum w, so a constant frame stays what it is.
// A miss pixel is not written. The last iteration (out != null) stores into the framebuffer:
// floats as they are, bytes as k_resolve_pixels quantizes them; alpha and row padding are
// not touched. DEMOD: the frames hold the demodulated signal d (k_atrous_load), every weight
// acts on d, and the last iteration stores d_n m with the modulation of mod4.
template <bool DEMOD>
__global__ __launch_bounds__(YRT_BLOCK) void k_atrous(AtrousParams ap, const float4* __restrict__ pos4,
                                                      const float4* __restrict__ nrm4, const float4* __restrict__ src,
                                                      float4* __restrict__ dst, FrameIO out,
                                                      const float4* __restrict__ mod4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ap.width * ap.height) return;
  const float INF = __int_as_float(0x7f800000);
  const float4 pp = pos4[i];
  if (!(pp.w < INF)) return;
  const int y = (int)(i / ap.width), x = (int)(i - (long long)y * ap.width);
  const float4 n4 = nrm4[i], c4 = src[i];
  const V3 xp = v3(pp.x, pp.y, pp.z), np = v3(n4.x, n4.y, n4.z), cp = v3(c4.x, c4.y, c4.z);
  const float rcpPlane = 1.0f / (ap.sigmaPosition * pp.w);
  V3 sum = v3s(0.f);
  float wsum = atrous_h(0) * atrous_h(0);
  for (int dy = -2; dy <= 2; ++dy) {
    const long long qy = (long long)y + (long long)dy * ap.step;
    if (qy < 0 || qy >= ap.height) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const long long qx = (long long)x + (long long)dx * ap.step;
      if (qx < 0 || qx >= ap.width || (dx == 0 && dy == 0)) continue;
      const size_t j = (size_t)qy * ap.width + (size_t)qx;
      const float4 pq = pos4[j];
      if (!(pq.w < INF)) continue;
      const float4 nq = nrm4[j], cq4 = src[j];
      const V3 d = v3(cq4.x, cq4.y, cq4.z) - cp;
      float w = atrous_h(dx) * atrous_h(dy);
      w = w * yrt_powf(fmaxf(0.f, dot(np, v3(nq.x, nq.y, nq.z))), ap.sigmaNormal);
      w = w * yrt_expf(-fabsf(dot(np, v3(pq.x, pq.y, pq.z) - xp)) * rcpPlane);
      if (ap.rcpSigmaColor2 > 0.f) w = w * yrt_expf(-dot(d, d) * ap.rcpSigmaColor2);
      sum = sum + w * d;
      wsum = wsum + w;
    }
  }
  V3 c = cp + sum * (1.0f / wsum);
  if (!out.pixels) {
    dst[i] = make_float4(c.x, c.y, c.z, 0.f);
    return;
  }
  if constexpr (DEMOD) {
    const float4 m = mod4[i];
    c = c * v3(m.x, m.y, m.z);
  }
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
    b = comp_sample<CM>(bs.c[0], mats, wo, dg, sx, sy, w, pdf);
    o[9] = pdf;
    o[10] = o[11] = 0.f;
  } else if (mode == 1) {
    uint32_t type = 0;
    a = set_sample<CM>(bs, mats, wo, dg, sx, sy, ss, b, pdf, type, st + threadIdx.x);
    o[6] = pdf;
    o[7] = __uint_as_float(type);
    o[8] = o[9] = o[10] = o[11] = 0.f;
  } else if (mode == 2) {
    camera_ray(*cam, r[0], r[1], a, b, sx, sy);
  } else {
    a = light_sample<kAllLights>(*light, dg, sx, sy, b, pdf);
    o[6] = pdf;
    o[7] = o[8] = o[9] = o[10] = o[11] = 0.f;
  }
  o[0] = a.x; o[1] = a.y; o[2] = a.z;
  o[3] = b.x; o[4] = b.y; o[5] = b.z;
  if (mode == 0) { o[6] = w.x; o[7] = w.y; o[8] = w.z; }
  if (mode == 2) o[6] = o[7] = o[8] = o[9] = o[10] = o[11] = 0.f;
}

// ---------------------------------------------------------------- BVH refit (faceCamera)
// Per-face dynamic geometry (rtUpdatePrimitive of YULIO_CAMERA_ALIGNED_ meshes,
// singleray_device.cpp:354-398) keeps the BVH topology and only moves vertices: the moved
// triangles' Moeller-Trumbore records are rewritten from the new world vertices, then the
// node boxes are refit bottom-up, one launch per tree level (deepest first). The reference
// rebuilt the whole Embree BVH on every face commit. Boxes stay the exact
// union of the original vertex bounds (what the builder computes), so the hits are identical
// to a rebuild's: the closest hit is the smallest (t, triangle id) whatever the tree.
__global__ __launch_bounds__(YRT_BLOCK) void k_refit_tris(GpuTri* __restrict__ tris, GpuTriShade* __restrict__ triShade,
                                                         const int4* __restrict__ indices,
                                                         const float4* __restrict__ positions,
                                                         const float4* __restrict__ normals,
                                                         const int* __restrict__ leafStart,
                                                         const int* __restrict__ leafSlots, int firstTri, int numTris) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numTris) return;
  const int gid = firstTri + i;
  const int4 ix = indices[gid];
  const float4 a = positions[ix.x], b = positions[ix.y], c = positions[ix.z];
  // the shading record's edges and vertex normals (scene_gpu.cpp builds it the same way)
  GpuTriShade& ts = triShade[gid];
  ts.e1[0] = a.x - b.x; ts.e1[1] = a.y - b.y; ts.e1[2] = a.z - b.z;
  ts.e2[0] = c.x - a.x; ts.e2[1] = c.y - a.y; ts.e2[2] = c.z - a.z;
  const float4 na = normals[ix.x], nb = normals[ix.y], nc = normals[ix.z];
  ts.n[0] = na.x; ts.n[1] = na.y; ts.n[2] = na.z;
  ts.n[3] = nb.x; ts.n[4] = nb.y; ts.n[5] = nb.z;
  ts.n[6] = nc.x; ts.n[7] = nc.y; ts.n[8] = nc.z;
  // every leaf slot referencing the triangle (spatial splits duplicate references)
  for (int k = leafStart[gid]; k < leafStart[gid + 1]; ++k) {
    GpuTri& t = tris[leafSlots[k]];
    // e1 = v0 - v1, e2 = v2 - v0 (device/bvh_build.cpp, rtcore convention); .w words kept
    t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
    t.e1[0] = a.x - b.x; t.e1[1] = a.y - b.y; t.e1[2] = a.z - b.z;
    t.e2[0] = c.x - a.x; t.e2[1] = c.y - a.y; t.e2[2] = c.z - a.z;
  }
}

__global__ __launch_bounds__(YRT_BLOCK) void k_refit_nodes(GpuNode* __restrict__ nodes, const GpuTri* __restrict__ tris,
                                                          const int4* __restrict__ indices,
                                                          const float4* __restrict__ positions,
                                                          const int* __restrict__ levelNodes, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  GpuNode& n = nodes[levelNodes[i]];
  for (int k = 0; k < 4; ++k) {
    const int c = n.child[k];
    if (c == -1) continue;
    const int idx = c >> 5, cnt = c & 31;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (cnt > 0) {
      for (int t = 0; t < cnt; ++t) {
        const int gid = __float_as_int(tris[idx + t].v0[3]);
        const int4 ix = indices[gid];
        const float4 p[3] = {positions[ix.x], positions[ix.y], positions[ix.z]};
        for (int v = 0; v < 3; ++v) {
          lo[0] = fminf(lo[0], p[v].x); hi[0] = fmaxf(hi[0], p[v].x);
          lo[1] = fminf(lo[1], p[v].y); hi[1] = fmaxf(hi[1], p[v].y);
          lo[2] = fminf(lo[2], p[v].z); hi[2] = fmaxf(hi[2], p[v].z);
        }
      }
    } else {
      const GpuNode& ch = nodes[idx];
      for (int j = 0; j < 4; ++j) {
        if (ch.child[j] == -1) continue;
        lo[0] = fminf(lo[0], ch.lox[j]); hi[0] = fmaxf(hi[0], ch.hix[j]);
        lo[1] = fminf(lo[1], ch.loy[j]); hi[1] = fmaxf(hi[1], ch.hiy[j]);
        lo[2] = fminf(lo[2], ch.loz[j]); hi[2] = fmaxf(hi[2], ch.hiz[j]);
      }
    }
    n.lox[k] = lo[0]; n.hix[k] = hi[0];
    n.loy[k] = lo[1]; n.hiy[k] = hi[1];
    n.loz[k] = lo[2]; n.hiz[k] = hi[2];
  }
}

__global__ __launch_bounds__(YRT_BLOCK) void k_quantize_nodes(const GpuNode* __restrict__ nodes,
                                                             GpuQNode* __restrict__ qnodes, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  GpuQNode q;
  yrt_quantize_node(nodes[i], q);  // the host builder's function: the same bytes
  qnodes[i] = q;
}

}  // namespace yrt
