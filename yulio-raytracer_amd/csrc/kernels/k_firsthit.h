// k_firsthit.h — the first-hit kernels off the render loop, the three callers of closest_hit
// (yrt_traverse.h): the debug renderer, rtPick and the guide pass (k_shade's post_intersect).
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
          h = closest_hit(sv.qnodes, sv.tris, org, dir, tnear, tfar);
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
            V3 e1, e2;
            yrt_tri_edges(&p0.x, &p1.x, &p2.x, &e1.x, &e2.x);
            V3 Nf = normalize(cross(e1, e2));  // ray.Ng
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

// SingleRayDevice::rtPick (api/singleray_device.cpp:692-708): one camera ray at image-plane
// (x, y), lens sample (0.5, 0.5), closest hit.
__global__ __launch_bounds__(YRT_TRACE_BLOCK) void k_pick(SceneView sv, const GpuCamera* camp, float x, float y,
                                                          float4* out) {
  if (threadIdx.x != 0) return;
  V3 org, dir;
  camera_ray(*camp, x, y, org, dir);
  const Hit h = closest_hit(sv.qnodes, sv.tris, org, dir, 0.f, __int_as_float(0x7f800000));
  const V3 p = org + h.t * dir;
  out[0] = make_float4(p.x, p.y, p.z, __int_as_float(h.tri));
}

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
// One view per face (a single frame is one face): blockIdx.y is the face, camp[face] its camera
// and the frames are [face][height][width] arrays.
template <bool ALBEDO>
__global__ __launch_bounds__(YRT_TRACE_BLOCK) void k_guides(SceneView sv, const GpuCamera* camp, int width, int height,
                                                            float4* __restrict__ pos4, float4* __restrict__ nrm4,
                                                            float4* __restrict__ albedo4) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)width * height) return;
  const int y = (int)(i / width), x = (int)(i - (long long)y * width);
  i += (long long)blockIdx.y * width * height;
  camp += blockIdx.y;
  V3 org, dir;
  camera_ray(*camp, (float(x) + 0.5f) / float(width), (float(y) + 0.5f) / float(height), org, dir);
  const Hit h = closest_hit(sv.qnodes, sv.tris, org, dir, 0.f, __int_as_float(0x7f800000));
  if (h.tri < 0) {
    pos4[i] = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7f800000));
    nrm4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (ALBEDO) albedo4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  DG dg;
  const float4* tsr = (const float4*)(sv.triShade + h.tri);
  const float4 r0 = tsr[0];
  const int g = __float_as_int(r0.w);  // geometry id rides in the shading record
  // the lazy record source: one pixel per thread, once per frame; the burst would only add registers
  post_intersect(sv, sv.geoms[g], TriRecordLazySource{tsr, r0}, org, dir, h.t, h.u, h.v, h.tri, dg, false, 0.f);
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

}  // namespace yrt
