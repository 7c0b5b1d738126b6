// k_shade.h — the shade kernel (environment, emission, continuation and shadow rays of one
// depth level) with its tunables and instruments, and the two resolves: k_shadow_resolve
// (unfused direct light) and k_resolve_pixels (sample sum, tone map, framebuffer).
#pragma once

#include "yrt_camera.h"
#include "yrt_surface.h"

namespace yrt {

// Occupancy target for k_shade. With the material / component / light cases pruned per
// instantiation (if constexpr), the Uber kernel needs 125 VGPRs: 4 waves/SIMD. Same box, C3:
// 3 waves 420.4, 4 waves 419.5, 5 waves 436.9 ms/frame (profiles/r02/shade_prune_r02.txt).
#ifndef YRT_SHADE_WAVES
#define YRT_SHADE_WAVES 4
#endif
#ifndef YRT_SHADE_WAVES_ALL
#define YRT_SHADE_WAVES_ALL 2  // the generic all-types instantiation (rare scenes): no spills at 2
#endif
#ifndef YRT_SHADE_WAVES_MP
#define YRT_SHADE_WAVES_MP YRT_SHADE_WAVES  // instantiations with MetallicPaint (C4's set)
#endif
// A hit vertex's loads in groups (profiles/shade_bursts_ab.txt), each switched off
// with -D...=0 and chosen per instantiation by the traits below:
//   YRT_SHADE_BURST_REC    the 96-byte GpuTriShade record in one group of six loads beside its
//                          first piece (TriRecordSource), before the geometry record is known
//   YRT_SHADE_BURST_GEOM   the geometry record's fields in one group (geom_burst)
//   YRT_SHADE_STORES_LAST  the continuation's and the first light's queue reservations together
//                          with no store in flight, the records' stores and pathL after them
#ifndef YRT_SHADE_BURST_REC
#define YRT_SHADE_BURST_REC 1
#endif
#ifndef YRT_SHADE_BURST_GEOM
#define YRT_SHADE_BURST_GEOM 1
#endif
#ifndef YRT_SHADE_STORES_LAST
#define YRT_SHADE_STORES_LAST 1
#endif
template <unsigned MM>
constexpr bool shade_burst_rec() { return YRT_SHADE_BURST_REC != 0; }
template <unsigned MM>
constexpr bool shade_burst_geom() { return YRT_SHADE_BURST_GEOM != 0; }
// not with MetallicPaint (C4's set): the continuation record kept live across the first light's
// term spills there (8 B of scratch at 128 VGPRs)
template <unsigned MM>
constexpr bool shade_stores_last() { return YRT_SHADE_STORES_LAST != 0 && !(MM & mat_bit(MAT_METALLIC_PAINT)); }

#ifdef YRT_PATH_DEBUG
// Debug builds only (-DYRT_PATH_DEBUG): per-vertex record of one path (pixel id, sample) of the
// shade kernel, 32 floats per depth, laid out as oracle_debug_path's (tools/c5_path_debug.py).
__device__ int g_dbgPath[2] = {-1, -1};
__device__ float g_dbgTrace[32 * 32];
#endif

template <unsigned MM>
__global__ __launch_bounds__(YRT_BLOCK) __attribute__((amdgpu_waves_per_eu(
    MM == (YRT_ALL_MATS | YRT_ALL_LIGHTS) ? YRT_SHADE_WAVES_ALL
    : (MM & mat_bit(MAT_METALLIC_PAINT)) ? YRT_SHADE_WAVES_MP
                                         : YRT_SHADE_WAVES))) void k_shade(SceneView sv, FrameView fv, PathBuffers pb, BatchInfo bi,
                                                   int depthLevel) {
#ifdef YRT_SHADE_PROF
  // shader-clock cycles per phase (wave-uniform points only), summed over the waves
  unsigned long long sprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev = __builtin_amdgcn_s_memtime();
#define SPROF_AT(k)                                            \
  do {                                                         \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    sprof[k] += t_ - tprev;                                    \
    tprev = t_;                                                \
  } while (0)
#endif
  // YRT_SHADE_PROF=1: one slot per phase; =2: the continuation and direct-light phases split
#if defined(YRT_SHADE_PROF) && YRT_SHADE_PROF == 1
#define SPROF_MARK(k) SPROF_AT(k)
#else
#define SPROF_MARK(k) ((void)0)
#endif
#if defined(YRT_SHADE_PROF) && YRT_SHADE_PROF == 2
#define SPROF_FINE(k) SPROF_AT(k)
#else
#define SPROF_FINE(k) ((void)0)
#endif
  const YRT_CONST GpuRenderParams& rp = const_ref(fv.rp);
  __shared__ QMap qm;
  __shared__ float sstash[7 * YRT_MAX_COMPS * YRT_BLOCK];  // set_sample candidates, [slot][lane]
  qmap_load(qm, pb.counters + qcounter_index(depthLevel, 0, 0), YRT_QSEGS);
  const int n = (int)qm.pre[YRT_QSEGS];
  const int cur = depthLevel & 1;
  const int numDirect = sv.numDirectLights;
  for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const unsigned ql = (unsigned)base + threadIdx.x;
    const bool active = (int)ql < n;
    const int q = active ? qmap_phys(qm, pb.segCap, ql) : 0;
    const int oseg = qseg_of((unsigned)base + (threadIdx.x & ~63u));
    unsigned* nextCount = pb.counters + qcounter_index(depthLevel + 1, 0, oseg);
    unsigned* shadowCount = pb.counters + qcounter_index(depthLevel, 1, oseg);
    int path = 0;
    V3 org = v3s(0.f), dir = v3s(0.f), thr = v3s(0.f), L = v3s(0.f);
    int meta = 0, depth = 0, rec = 0, pixelId = 0, s = 0, medium = 0;
    bool ignoreVL = false, unbent = false, isHit = false, useDirect = false;
    bool haveL = false;  // L holds pathL[path] plus this vertex's emission (written back below)
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    DG dg;
    BRDFSet bs;
    bs.n = 0;
#pragma unroll
    for (int k = 0; k < YRT_MAX_COMPS; ++k) {
      bs.c[k].kind = 0;
      bs.c[k].R = v3s(0.f);
      bs.c[k].a = bs.c[k].b = bs.c[k].c = 0.f;
    }
    V3 wo = v3s(0.f);
    int px = 0, py = 0;
    SPROF_MARK(7);
    SPROF_FINE(7);
    if (active) {
      path = pb.qPath[cur][q];
      h = pb.hit[q];
      if (depthLevel == 0) {
        // camera rays (k_raygen): throughput 1, depth 0, unbent, vacuum, zero radiance so far;
        // pathL is written below for every queued path
        thr = v3s(1.f);
        meta = 1 << 9;
        L = v3s(0.f);
        haveL = true;
      } else {
        const float4 t4 = pb.qThr[cur][q];
        thr = v3(t4.x, t4.y, t4.z);
        meta = __float_as_int(t4.w);
      }
      depth = meta & 255;
      ignoreVL = (meta >> 8) & 1;
      unbent = (meta >> 9) & 1;
      medium = (meta >> 10) & 0xFFFF;  // LightPath::lastMedium as a medium-table index
      s = fastdiv(path, bi.divPixels);
      const int i = path - s * bi.numPixels;
      batch_pixel(rp, bi, i, px, py, (const int*)pb.reserved);
      pixelId = py * rp.width + px;
      isHit = __float_as_int(h.w) >= 0;
    }
    // the ray's direction, origin and sample record are read where they are used: a miss
    // reads the direction only for an emitting environment light whose Le depends on it, and
    // neither the origin nor the sample record unless it looks up the backplate (a hit issues
    // these loads beside its shading record's, off its dependent chain)
    if (active && (isHit || sv.numEnvDir > 0)) {
      const float4 d = pb.qDir[cur][q];
      dir = v3(d.x, d.y, d.z);
      wo = -dir;
    }
    SPROF_MARK(0);  // queue record, pixel and sample record
    if (active && !isHit) {
      {
        const int x = px, y = py;
        // environment shading (pathtraceintegrator.cpp:79-92): the backplate for a straight
        // camera ray, looked up at the sample's image-plane position (state.pixel)
        if (fv.backplateTexels && unbent) {
          rec = fv.pixelSets[pixelId] * rp.spp + s;
          const float fx = (float(x) + samp(fv, 0, rec)) * rp.rcpWidth;
          const float fy = (float(y) + samp(fv, 1, rec)) * rp.rcpHeight;
          const GpuImage& bp = fv.backplate;
          const int bx = max(0, min((int)(fx * (float)bp.width), bp.width - 1));
          const int by = max(0, min((int)(fy * (float)bp.height), bp.height - 1));
          float c[4];
          texel(bp, fv.backplateTexels, bx, by, c);
          if (!haveL) { const float4 l4 = pb.pathL[path]; L = v3(l4.x, l4.y, l4.z); haveL = true; }
          L = L + thr * v3(c[0], c[1], c[2]);
        } else if (!ignoreVL) {
          for (int j = 0; j < sv.numEnvLights; ++j) {
            if (!haveL) { const float4 l4 = pb.pathL[path]; L = v3(l4.x, l4.y, l4.z); haveL = true; }
            L = L + thr * env_Le<lights_of<MM>()>(sv, const_ref(sv.lights + const_ref(sv.envLights + j)), wo);
          }
          // the zero environment lights' throughput * 0: a no-op unless the throughput is not
          // finite, where the reference's add makes the radiance NaN
          if (sv.numEnvZero > 0 && !(fabsf(thr.x) <= 3.40282347e38f && fabsf(thr.y) <= 3.40282347e38f && fabsf(thr.z) <= 3.40282347e38f)) {
            if (!haveL) { const float4 l4 = pb.pathL[path]; L = v3(l4.x, l4.y, l4.z); haveL = true; }
            L = L + thr * v3s(0.f);
          }
        }
      }
    }
    SPROF_MARK(1);  // misses: environment / backplate
    bool backfacing = false;
    int g = 0;  // the hit's geometry (sv.geomRecs)
    // the geometry record's material and tex[0] descriptor in registers (geom_burst)
    GpuMaterial gm = {};
    GpuTexture gt0 = {};
    if (active && isHit) {
      const int gid = __float_as_int(h.w);
      const float4* tsr = (const float4*)(sv.triShade + gid);
      // The whole record beside its first piece: the five other addresses are known with the hit,
      // the geometry record (which says what of it the mesh reads) only after r[0]. In bounds for
      // every hit: a hit's id is a global triangle id, and triShade holds one full 96-byte record
      // per global triangle id, whatever its geometry's kind (scene_gpu.cpp sizes it by the index
      // array, which spheres, disks and `triangle` shapes are tessellated into); r[0] is read for
      // every hit already. GEOM_TRIANGLE and the indexed source ignore the other 80 bytes.
      TriRecordSource trs;
      trs.r[0] = tsr[0];
      if constexpr (shade_burst_rec<MM>()) {
#pragma unroll
        for (int k = 1; k < 6; ++k) trs.r[k] = tsr[k];
      }
      const float4 r0 = trs.r[0];
      const float4 o = pb.qOrg[cur][q];
      org = v3(o.x, o.y, o.z);
      rec = fv.pixelSets[pixelId] * rp.spp + s;
      g = __float_as_int(r0.w);  // geometry id rides in the shading record
      const float time = pb.qTime[0] ? samp(fv, 4, rec) : 0.f;
      // tangents only feed the Obj bump map and the anisotropic microfacet
      auto want_tangents = [&](int mat, const GpuMaterial& m) {
        return mat >= 0 && (((MM & mat_bit(MAT_OBJ)) && m.type == MAT_OBJ && m.tex[4] >= 0) ||
                            ((MM & mat_bit(MAT_BRUSHED_METAL)) && m.type == MAT_BRUSHED_METAL));
      };
      auto post = [&](const auto& geom, bool wantT) {
        if constexpr (shade_burst_rec<MM>())
          post_intersect(sv, geom, trs, org, dir, h.x, h.y, h.z, gid, dg, wantT, time);
        else
          post_intersect(sv, geom, TriRecordLazySource{tsr, r0}, org, dir, h.x, h.y, h.z, gid, dg, wantT, time);
      };
      if constexpr (shade_burst_geom<MM>()) {
        GeomHead gh;
        geom_burst<MM>(sv.geomRecs + g, gh, gm, gt0);
        post(gh, want_tangents(gh.material, gm));
      } else {
        const GpuGeomRec& gr = sv.geomRecs[g];
        post(gr.g, want_tangents(gr.g.material, gr.m));
      }
      if (dot(dg.Ng, dir) > 0.f) {
        backfacing = true;
        dg.Ng = -dg.Ng;
        dg.Ns = -dg.Ns;
      }
    }
    SPROF_MARK(2);  // postIntersect
    if (active && isHit) {
      if (dg.material >= 0) {
        if constexpr (shade_burst_geom<MM>()) shade_material<MM>(sv, gm, gt0, dg.material, medium, dg, bs);
        else shade_material<MM>(sv, sv.geomRecs[g].m, sv.geomRecs[g].t0, dg.material, medium, dg, bs);
      }
      if (!ignoreVL && dg.light >= 0 && !backfacing) {
        const GpuLight& al = sv.lights[dg.light];
        if (!haveL) { const float4 l4 = pb.pathL[path]; L = v3(l4.x, l4.y, l4.z); haveL = true; }
        L = L + thr * v3(al.L[0], al.L[1], al.L[2]);
      }
#pragma unroll
      for (int k = 0; k < YRT_MAX_COMPS; ++k)
        if (k < bs.n) useDirect |= (comp_type(bs.c[k].kind) & BT_DIFFUSE) != 0;
      dg_frame(dg);
    }
    SPROF_MARK(3);  // material::shade (textures), emission

    // continuation (pathtraceintegrator.cpp:169-213)
    bool cont = false;
    V3 nwi = v3s(0.f), nthr = v3s(0.f);
    int nmeta = 0;
    bool doSample = false;
    float4 sd = make_float4(0.f, 0.f, 0.f, 0.f);
    float sy = 0.f, ss = 0.f;
    if (active && isHit) {
      bool stop = depth >= rp.maxDepth - 1;
      if (!stop && rp.rrDepth > 0 && depth >= rp.rrDepth - 1) {  // size_t compare in the reference
        const float qrr = fminf(reduce_max(thr) * 1.f * 1.f, .95f);  // eta == 1
        if (samp(fv, 5 + rp.firstScatterTypeSampleID + depth, rec) >= qrr) stop = true;
      }
      if (!stop) {
        const int d2 = rp.firstScatterSampleID + depth;
        // the 2-D sample's tabulated terms in place of its first coordinate; the second one
        // only where a power-cosine sampler can read it
        sd = samp_dir(fv, d2, rec);
        if constexpr ((comps_of(MM) & kCompsRawSy) != 0u) sy = samp(fv, 5 + rp.dim1D + 2 * d2 + 1, rec);
        ss = samp(fv, 5 + rp.firstScatterTypeSampleID + depth, rec);
        doSample = true;
      }
    }
    SPROF_FINE(0);  // everything before CompositedBRDF::sample
    float spdf = 0.f;
    uint32_t stype = 0;
    V3 sc = v3s(0.f);
    if (doSample)
      sc = set_sample<comps_of(MM)>(bs, sv.materials, wo, dg, sd, sy, ss, nwi, spdf, stype, sstash + threadIdx.x);
    SPROF_FINE(1);  // CompositedBRDF::sample
    if (doSample) {
      {
        V3 c = sc;
        const float pdf = spdf;
        const uint32_t type = stype;
        if (!(c == v3s(0.f) || pdf <= 0.f)) {
          if (MM & mat_bit(MAT_DIELECTRIC)) {
            // simple volumetric effect and medium tracking (pathtraceintegrator.cpp:197-207)
            const float4 T = sv.media[medium];
            if (!(T.x == 1.f && T.y == 1.f && T.z == 1.f)) c = c * v3(yrt_powf(T.x, h.x), yrt_powf(T.y, h.x), yrt_powf(T.z, h.x));
            if ((type & BT_TRANSMISSION) && dg.material >= 0) {
              const GpuMaterial& mt = sv.materials[dg.material];
              if (mt.type == MAT_DIELECTRIC) medium = medium == mt.media[1] ? mt.media[0] : mt.media[1];
            }
          }
          nthr = thr * c * rcpf_(pdf);
          const bool nIgnore = (type & BT_DIFFUSE) != 0;
          const bool nUnbent = unbent && (nwi == dir);
          // loop head of the next iteration: depth+1 < maxDepth holds; minContribution test
          if (!(reduce_max(nthr) < rp.minContribution)) {
            cont = true;
            nmeta = (depth + 1) | ((nIgnore ? 1 : 0) << 8) | ((nUnbent ? 1 : 0) << 9) | (medium << 10);
          }
        }
      }
    }
    SPROF_MARK(4);  // continuation: CompositedBRDF::sample, Russian roulette
    // pathL[path]: nothing in this kernel reads it after this point, so where it is stored is
    // free. A store counts in the same counter as the loads and the atomics' returns: stored
    // here, the continuation's reservation below waits for its acknowledgement as well.
    if constexpr (!shade_stores_last<MM>())
      if (haveL) pb.pathL[path] = make_float4(L.x, L.y, L.z, 0.f);
    // the continuation's records (pathtraceintegrator.cpp:169-213) at queue slot nq
    auto cont_store = [&](unsigned nq) {
      if (pb.qTime[0]) pb.qTime[cur ^ 1][nq] = samp(fv, 4, rec);  // lastRay.time (:210)
      pb.qPath[cur ^ 1][nq] = path;
      pb.qOrg[cur ^ 1][nq] = make_float4(dg.P.x, dg.P.y, dg.P.z, dg.error * rp.epsilon);
      pb.qDir[cur ^ 1][nq] = make_float4(nwi.x, nwi.y, nwi.z, __int_as_float(0x7f800000));
      pb.qThr[cur ^ 1][nq] = make_float4(nthr.x, nthr.y, nthr.z, __int_as_float(nmeta));
    };
    // direct lighting: one shadow ray per light (pathtraceintegrator.cpp:123-167); its
    // contribution is added to pathL[path] after the emission above (reference order)
    auto light_term = [&](int k, V3& wi, float& tfar, V3& contrib) -> bool {
      const int li = const_ref(sv.directLights + k);
      const YRT_CONST GpuLight& lt = const_ref(sv.lights + li);  // scalar loads
      const bool lit = active && isHit && useDirect && (lt.illumMask & dg.illumMask) != 0;
      V3 Ls = v3s(0.f);
      float pdf = 0.f;
      if (lit) {
        if (lt.precomputed >= 0) {
          const float* ls = fv.lightSamples + ((size_t)rec * fv.numLightSlots + lt.precomputed) * 8;
          wi = v3(ls[0], ls[1], ls[2]);
          pdf = ls[3];
          Ls = v3(ls[4], ls[5], ls[6]);
        } else {
          // the light's type is wave-uniform: the dome light loads the sample's tabulated terms,
          // the triangle light its raw coordinates, the distant light both
          float4 lsd = make_float4(0.f, 0.f, 0.f, 0.f);
          float lsx = 0.f, lsy = 0.f;
          if ((1u << lt.type) & kLightsDir) lsd = samp_dir(fv, rp.lightSampleID, rec);
          if ((lights_of<MM>() & kLightsRawS) != 0u && ((1u << lt.type) & kLightsRawS)) {
            lsx = samp(fv, 5 + rp.dim1D + 2 * rp.lightSampleID, rec);
            lsy = samp(fv, 5 + rp.dim1D + 2 * rp.lightSampleID + 1, rec);
          }
          Ls = light_sample<lights_of<MM>()>(lt, dg, lsd, lsx, lsy, wi, pdf);
        }
      }
      SPROF_FINE(3);  // Light::sample
      const bool lsOk = lit && !(Ls == v3s(0.f) || pdf == 0.f);
      V3 brdf = v3s(0.f);
      if (lsOk) brdf = set_eval<comps_of(MM)>(bs, sv.materials, wo, dg, wi, BT_DIFFUSE);
      SPROF_FINE(4);  // CompositedBRDF::eval
      if (lsOk && !(brdf == v3s(0.f))) {
        const float r01 = hash_u01(rp.frameSeed, (uint32_t)pixelId, (uint32_t)s, (uint32_t)(depth * 64 + li));
        const float shadowRayJitterLength = 2.f * rp.tMaxShadowRay * rp.tMaxShadowJitter * r01 -
                                            rp.tMaxShadowRay * rp.tMaxShadowJitter;
        float tMax = rp.tMaxShadowRay + shadowRayJitterLength;
        const float dotProduct = dot(wi, ld3(rp.up));
        if (dotProduct <= 0.f) tMax += rp.tMaxShadowRay * 100.f * smoothstepf(0.f, 1.f, fabsf(dotProduct));
        tfar = tMax - dg.error * rp.epsilon;
        contrib = thr * Ls * brdf * rcpf_(pdf);
        return true;
      }
      return false;
    };
    // shadow ray records at slot si: origin (dg.P, dg.error * epsilon), direction and tfar, the
    // light's contribution and the path id
    auto shadow_store = [&](unsigned si, const V3& wi, float tfar, const V3& contrib) {
      if (pb.sTime) pb.sTime[si] = samp(fv, 4, rec);  // lastRay.time (:158)
      pb.sOrg[si] = make_float4(dg.P.x, dg.P.y, dg.P.z, dg.error * rp.epsilon);
      pb.sDir[si] = make_float4(wi.x, wi.y, wi.z, tfar);
      pb.sContrib[si] = make_float4(contrib.x, contrib.y, contrib.z, __int_as_float(path));
    };
    auto shadow_append = [&](int k, bool pred, const V3& wi, float tfar, const V3& contrib) {
      bool sgot;
      const unsigned si = oseg * pb.shSegCap + wave_append(shadowCount, pred, sgot);
      if (sgot) shadow_store(si, wi, tfar, contrib);
      if (active && !pb.fuseShadow) pb.shFirst[(size_t)q * numDirect + k] = sgot ? (int)si : -1;
    };
    if constexpr (shade_stores_last<MM>()) {
      // The first light's term is worked out before either reservation (it stores nothing), the
      // two reservations go out together with no store in flight, and every store of the vertex
      // follows them: a slot is written only after its reservation has returned, as before. The
      // continuation record stays live across the first light's term.
      V3 wi = v3s(0.f), contrib = v3s(0.f);
      float tfar = 0.f;
      const bool pred = numDirect > 0 && light_term(0, wi, tfar, contrib);
      SPROF_FINE(5);
      unsigned nq, si;
      wave_append2(nextCount, cont, nq, shadowCount, pred, si);
      nq += oseg * pb.segCap;
      si += oseg * pb.shSegCap;
      if (cont) cont_store(nq);
      SPROF_MARK(5);
      SPROF_FINE(2);
      if (numDirect > 0) {
        if (pred) shadow_store(si, wi, tfar, contrib);
        if (active && !pb.fuseShadow) pb.shFirst[(size_t)q * numDirect] = pred ? (int)si : -1;
      }
      SPROF_FINE(6);
      for (int k = 1; k < numDirect; ++k) {
        const bool predk = light_term(k, wi, tfar, contrib);
        SPROF_FINE(5);
        shadow_append(k, predk, wi, tfar, contrib);
        SPROF_FINE(6);
      }
      if (haveL) pb.pathL[path] = make_float4(L.x, L.y, L.z, 0.f);
    } else {
      bool got;
      const unsigned nq = oseg * pb.segCap + wave_append(nextCount, cont, got);
      if (got) cont_store(nq);
      SPROF_MARK(5);  // continuation append and stores
      SPROF_FINE(2);  // rest of the continuation, append and stores
      for (int k = 0; k < numDirect; ++k) {
        V3 wi = v3s(0.f), contrib = v3s(0.f);
        float tfar = 0.f;
        const bool pred = light_term(k, wi, tfar, contrib);
        SPROF_FINE(5);  // shadow-ray jitter, contribution
        shadow_append(k, pred, wi, tfar, contrib);
        SPROF_FINE(6);  // shadow-ray append and stores
      }
    }
    SPROF_MARK(6);  // direct light: light sample, BRDF eval, shadow-ray append and stores
#ifdef YRT_PATH_DEBUG
    if (active && pixelId == g_dbgPath[0] && s == g_dbgPath[1] && depth < 32) {
      float* o = g_dbgTrace + depth * 32;
      if (!haveL) { const float4 l4 = pb.pathL[path]; L = v3(l4.x, l4.y, l4.z); }
      const float r[32] = {1.f, isHit ? (float)__float_as_int(h.w) : -1.f, h.x, h.y, h.z, thr.x, thr.y, thr.z,
                           dg.P.x, dg.P.y, dg.P.z, dg.Ns.x, dg.Ns.y, dg.Ns.z, L.x, L.y, L.z, nwi.x, nwi.y, nwi.z,
                           spdf, sc.x, sc.y, sc.z, nthr.x, nthr.y, nthr.z, dir.x, dir.y, dir.z, org.x, (float)useDirect};
      for (int k = 0; k < 32; ++k) o[k] = r[k];
    }
#endif
  }
#ifdef YRT_SHADE_PROF
  if (threadIdx.x == 0)
    for (int k = 0; k < 8; ++k) atomicAdd(&g_traceProfile[k], sprof[k]);
#endif
}

// Adds the unoccluded direct-light terms in light order.
__global__ __launch_bounds__(YRT_BLOCK) void k_shadow_resolve(PathBuffers pb, int depthLevel, int numLights) {
  __shared__ QMap qm;
  qmap_load(qm, pb.counters + qcounter_index(depthLevel, 0, 0), YRT_QSEGS);
  const int n = (int)qm.pre[YRT_QSEGS];
  const int cur = depthLevel & 1;
  for (int ql = blockIdx.x * blockDim.x + threadIdx.x; ql < n; ql += gridDim.x * blockDim.x) {
    const int q = qmap_phys(qm, pb.segCap, (unsigned)ql);
    bool any = false;
    for (int li = 0; li < numLights; ++li) any |= pb.shFirst[(size_t)q * numLights + li] >= 0;
    if (!any) continue;
    float4* Lp = &pb.pathL[pb.qPath[cur][q]];
    const float4 l4 = *Lp;
    V3 L = v3(l4.x, l4.y, l4.z);
    for (int li = 0; li < numLights; ++li) {
      const int si = pb.shFirst[(size_t)q * numLights + li];
      if (si < 0 || pb.sOcc[si]) continue;
      const float4 c = pb.sContrib[si];
      L = L + v3(c.x, c.y, c.z);
    }
    *Lp = make_float4(L.x, L.y, L.z, 0.f);
  }
}

// Debug capture (yrtDebugPixelSamples): the per-sample radiance of one pixel of one frame,
// in the pixel's summation order, for parity debugging against oracle_debug_pixel.
__device__ int g_dbgPixel[3] = {-1, -1, 0};  // pixel id (y * width + x), frame, capacity of g_dbgOut
__device__ float4* g_dbgOut = nullptr;

// AccuBuffer::update (api/framebuffer.h:289-304) + DefaultToneMapper::eval
// (tonemappers/defaulttonemapper.h:23-49) + FrameBufferRGB8::set (api/framebuffer.h:220-226)
__global__ __launch_bounds__(YRT_BLOCK) void k_resolve_pixels(FrameView fv, PathBuffers pb, BatchInfo bi,
                                                            float* __restrict__ fbFloat, uint8_t* __restrict__ fbRGB8,
                                                            int rgb8Stride, float4* __restrict__ accu, int accumulate) {
  const YRT_CONST GpuRenderParams& rp = const_ref(fv.rp);
  const size_t frameStride = (size_t)rp.width * rp.height;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < bi.numPixels; i += gridDim.x * blockDim.x) {
    int x, y, f;
    if (!batch_pixel(rp, bi, i, x, y, f, (const int*)pb.reserved)) continue;
    V3 L = v3s(0.f);
    for (int s = 0; s < rp.spp; ++s) {
      const float4 l4 = pb.pathL[(size_t)s * bi.numPixels + i];
      L = L + v3(l4.x, l4.y, l4.z);
    }
    if (g_dbgPixel[0] == y * rp.width + x && g_dbgPixel[1] == f && g_dbgOut)
      for (int s = 0; s < min(rp.spp, g_dbgPixel[2]); ++s) g_dbgOut[s] = pb.pathL[(size_t)s * bi.numPixels + i];
    // AccuBuffer::update: non-accumulating frames store (L, spp), accumulating ones add
    const size_t pix = (size_t)f * frameStride + (size_t)y * rp.width + x;
    float4 a = make_float4(L.x, L.y, L.z, (float)rp.spp);
    if (accumulate) {
      const float4 c = accu[pix];
      a = make_float4(c.x + L.x, c.y + L.y, c.z + L.z, c.w + (float)rp.spp);
    }
    accu[pix] = a;
    V3 L0 = accumulate ? v3(a.x, a.y, a.z) * rcpf_(a.w) : L * rcpf_((float)rp.spp);
    if (rp.gamma != 1.0f) L0 = v3(yrt_powf(L0.x, rp.rcpGamma), yrt_powf(L0.y, rp.rcpGamma), yrt_powf(L0.z, rp.rcpGamma));
    if (rp.vignetting) {
      // DefaultToneMapper::eval's vignette (tonemappers/defaulttonemapper.h:44-49), after the gamma
      const float rw = rcpf_(0.5f * float(rp.width));
      const float vx = (float(x) - 0.5f * float(rp.width)) * rw, vy = (float(y) - 0.5f * float(rp.height)) * rw;
      const float d = sqrtf(vx * vx + vy * vy);
      L0 = L0 * yrt_powf(yrt_cosf(d * 0.5f), 3.0f);
    }
    if (fbFloat) {
      float* o = fbFloat + pix * 3;
      o[0] = L0.x;
      o[1] = L0.y;
      o[2] = L0.z;
    }
    if (fbRGB8) {
      uint8_t* o = fbRGB8 + ((size_t)f * rp.height + y) * rgb8Stride + 3 * x;
      o[0] = (uint8_t)clampf(L0.x * 255.0f, 0.0f, 255.0f);
      o[1] = (uint8_t)clampf(L0.y * 255.0f, 0.0f, 255.0f);
      o[2] = (uint8_t)clampf(L0.z * 255.0f, 0.0f, 255.0f);
    }
  }
}

#undef SPROF_AT
#undef SPROF_MARK
#undef SPROF_FINE

}  // namespace yrt
