// k_trace.h — the ray-query kernel (closest hit, any hit, and the fused depth-0 camera-ray
// instantiation) with its tunables.
#pragma once

#include "yrt_camera.h"
#include "yrt_traverse.h"
#include "../common/yrt_tri_record.h"

namespace yrt {

// Ray-query kernel with lane refill (persistent-wave traversal, after Aila & Laine 2009):
// each wave owns a contiguous chunk of the queue; the traversal advances one node visit or
// one leaf per iteration, and whenever at least YRT_REFILL lanes of the wave have finished
// their ray, those lanes take the next rays of the chunk (ballot + popcount, no atomics).
// This keeps 64-wide waves busy although ray costs differ by 10-100x. Same visit order and
// the same (t, triangle id) closest-hit rule as closest_hit (yrt_traverse.h).
// Nothing global is loaded and waited for between the loop head and the node / leaf step: what
// a finished query owes to memory is paid at the refill, in one batch for the refilling lanes —
// closest hit stores its hit record there; any hit with the fused shadow resolve adds its
// unoccluded rays' light there (shadow_done; profiles/shadow_resolve_at_refill.txt).
#ifndef YRT_REFILL
#define YRT_REFILL 40  // 24/6 +1.3 % over 16/4; with 64-lane blocks 28/6 +0.4 %, then 40/8 +0.9 % over 28/6;
                        // with four lanes 48 everywhere: C4 -0.8 %, C3 +0.2 %, C5 +1.6 % (r05cc/dd/ee)
#endif
#ifndef YRT_REFILL_ANY
#define YRT_REFILL_ANY 32  // any hit: with node bias 20, C3 +1.5 %, C4 / C5 within the spread (r05ii); with the
                           // resolve at the refill 24 loses 1.7 ms on C3, 40 is within the spread (-0.3 ms)
#endif
#ifndef YRT_REFILL_PRIM
#define YRT_REFILL_PRIM YRT_REFILL  // refill threshold of the fused depth-0 instantiation
#endif
constexpr int kTriStep = 2;  // triangles per lane per leaf step: 2 is +0.7 % over whole leaves
#ifndef YRT_TRI_STEP_ANY
#define YRT_TRI_STEP_ANY kTriStep  // any-hit: triangles per lane per leaf step (sequential, early exit)
#endif
#ifndef YRT_NODE_BIAS
#define YRT_NODE_BIAS 8  // node step iff lanes at a node * 4 > blocked lanes * YRT_NODE_BIAS
#endif
// Every instantiation traverses the 64-B quantized nodes (common/yrt_qnode.h), which give the
// same query results as the 128-B float nodes bit for bit (conservative boxes).
// Closest hit: neutral at a 32-entry LDS ring (LDS-bound 4.75 waves/SIMD); with a 16-entry ring
// the quantized kernel runs 74 VGPRs at 6 waves/SIMD and the smaller node footprint pays for the
// extra waves' cache interference that the float nodes lose to (same box, profiles/r06/
// ab_r06j.txt: C3 +5.3 %, C4 -1.8 %, C5 -2.5 %; float nodes with the 16-entry ring C3 -2 %).
#ifndef YRT_NODE_BIAS_ANY
#define YRT_NODE_BIAS_ANY 20  // any hit: 12 over 8 -1.7 % on C3, C5 within the spread (r03 anyk); 4 +2.4 %;
                              // four lanes (r05gg-ii): 24 / 32 C3 -2.0 / -2.8 % but C5 +1.6 / +2.3 %
                              // unless refill 32 (20 / 32: C3 -1.5 %, C5 +0.0 %)
#endif
#ifndef YRT_TRACE_WAVES
// 6: a scheduling target — the 16 KB LDS stack of a 128-lane block holds the kernels at 5
// waves/SIMD, but code scheduled for 6 (78/74 VGPRs with SGPR-based node addressing) runs
// +0.6 % on C3 over code scheduled for 5 (profiles/r01/variants_r01.txt)
#define YRT_TRACE_WAVES 6
#endif
#ifndef YRT_TRACE_WAVES_PRIM
// the camera-ray (fused depth-0) instantiations: register target of 5 waves/SIMD (96 VGPRs)
#define YRT_TRACE_WAVES_PRIM 5
#endif
#ifndef YRT_TRACE_WAVES_ANY
// occupancy target of the shadow-ray instantiation: 8 waves/SIMD (64 VGPRs, no scratch; the
// 16-entry LDS ring allows 9): same box against 7 (profiles/r06/ab_r06g.txt) C3 +1.9 / +0.8 %,
// C4 -0.7 / -1.1 %, C5 -1.4 %
#define YRT_TRACE_WAVES_ANY 8
#endif
#ifdef YRT_PROFILE
#ifndef YRT_PROFILE_ANY
#define YRT_PROFILE_ANY 0  // which instantiation counts: 0 closest hit, 1 any hit
#endif
#define YRT_PROF(i, v) (ANY == (YRT_PROFILE_ANY != 0) ? (void)(prof[i] += (unsigned long long)(v)) : (void)0)
#else
#define YRT_PROF(i, v) ((void)0)
#endif

// A finished shadow query. Not fused: its occlusion flag is stored. Fused (PathBuffers::
// fuseShadow, one light): an unoccluded ray's contribution is added to its path's radiance
// (k_shadow_resolve's operations), but not here: the lane keeps its slot in q ("pending") and
// the kernel resolves it at its next refill or at the wave's end, as the closest-hit
// instantiation stores its hits; q = -1: occluded, nothing to add. The two dependent loads of
// the sum (contrib[q], then pathL[contrib[q].w]) miss L2, and waited for here, inside the
// traversal loop, they would stop the lanes still traversing once per unoccluded ray.
__device__ __forceinline__ void shadow_done(const ShadowFuse& sf, int* __restrict__ occOut, int& q, bool occluded) {
  if (sf.contrib) {
    if (occluded) q = -1;
  } else {
    occOut[q] = occluded ? 1 : 0;
    q = -1;
  }
}

// A leaf triangle as tested at ray time t: static scenes read the GpuTri as stored; moving
// scenes (MOTION) rebuild v0, e1, e2 from p + t * m (trianglemesh_full.cpp:104-109, the same
// operations as the oracle's trace), keeping the record's id and flag words.
template <bool MOTION>
__device__ __forceinline__ GpuTri tri_at(const GpuTri* __restrict__ tris, const GpuTriMotion* __restrict__ tms,
                                         int slot, float time) {
  GpuTri t = tris[slot];
  if constexpr (MOTION) {
    const GpuTriMotion m = tms[slot];
    float p0[3], p1[3], p2[3];
    for (int k = 0; k < 3; ++k) p0[k] = t.v0[k] + time * m.m0[k];
    for (int k = 0; k < 3; ++k) p1[k] = m.p1[k] + time * m.m1[k];
    for (int k = 0; k < 3; ++k) p2[k] = m.p2[k] + time * m.m2[k];
    yrt_tri_vertices(t, p0, p1, p2);
  }
  return t;
}

// MOTION: moving geometry; rayTime[q] is query q's time (Ray::time, set from sample.getTime()
// for camera rays and inherited by shadow and continuation rays, pathtraceintegrator.cpp:158,210)
// PRIM = 1 (closest hit, static scenes): depth 0 from the batch's path ids instead of a queue —
// camera rays generated at refill, hits appended to the depth-0 queue, misses resolved
// (PrimaryRays)
template <bool ANY, bool MOTION, int PRIM = 0>
__global__ __launch_bounds__(YRT_TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(
    ANY ? YRT_TRACE_WAVES_ANY : PRIM ? YRT_TRACE_WAVES_PRIM : YRT_TRACE_WAVES))) void k_trace(
    SceneView sv, const float4* __restrict__ org,
                                                         const float4* __restrict__ dir,
                                                         const unsigned* __restrict__ counts, int numSegs,
                                                         int segCap, float4* __restrict__ hitOut,
                                                         int* __restrict__ occOut, int* __restrict__ spillBuf,
                                                         ShadowFuse sf, const float* __restrict__ rayTime,
                                                         PrimaryRays pr) {
  static_assert(!PRIM || (!ANY && !MOTION), "camera rays: closest hit, static scenes");
  constexpr int kLds = ANY ? YRT_LDS_STACK_ANY : PRIM ? YRT_LDS_STACK_PRIM : YRT_LDS_STACK;
  __shared__ int lstack[kLds * YRT_TRACE_BLOCK];
  __shared__ QMap qm;
  unsigned n;
  if constexpr (PRIM) {
    n = (unsigned)pr.bi.numPixels * (unsigned)const_ref(pr.fv.rp).spp;
  } else {
    qmap_load(qm, counts, numSegs);
    n = qm.pre[YRT_QSEGS];
  }
  const int lane = lane_id();
  const unsigned wavesPerBlock = YRT_TRACE_BLOCK / 64;
  const unsigned gw = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6);
  const unsigned numWaves = gridDim.x * wavesPerBlock;
  unsigned chunk = (n + numWaves - 1) / numWaves;
  chunk = chunk < 64u ? 64u : chunk;
  unsigned next = gw * chunk;
  const unsigned end = min(n, next + chunk);
  if (next >= end) return;  // wave-uniform

  const GpuQNode* __restrict__ qnodes = sv.qnodes;
  const GpuTri* __restrict__ tris = sv.tris;
  int* stack = lstack + threadIdx.x;
  // Deep stack entries (rare) spill to global memory, [entry][thread]: a private array here
  // would let the compiler fuse LDS and scratch pops into one slow flat load.
  const size_t spillStride = (size_t)gridDim.x * YRT_TRACE_BLOCK;
  int* __restrict__ spill = spillBuf + blockIdx.x * YRT_TRACE_BLOCK + threadIdx.x;

  bool has = false;
  // cur: next entry to process (count 0 = inner node, >0 = leaf range, -1 = stack exhausted)
  // pend: a leaf parked during the inner-node phase (count 0 = none)
  int q = 0, sp = 0, curIdx = 0, curCnt = 0, pendIdx = 0, pendCnt = 0;
  // The LDS stack is a ring holding the top YRT_LDS_STACK entries; older entries are evicted
  // to global memory on push and restored into the freed slot on pop (both rare). Every pop
  // returns an LDS value, so the hot path stays a ds_read.
#define YRT_SLOT(i) ((((i) & (kLds - 1))) * YRT_TRACE_BLOCK)
#define YRT_POP_READ(e_)                                                          \
  do {                                                                            \
    e_ = (unsigned)stack[YRT_SLOT(sp)];                                           \
    if (sp >= kLds) stack[YRT_SLOT(sp)] = spill[(size_t)(sp - kLds) * spillStride]; \
  } while (0)
#define YRT_PUSH(e)                                                               \
  do {                                                                            \
    if (sp >= kLds) spill[(size_t)(sp - kLds) * spillStride] = stack[YRT_SLOT(sp)]; \
    stack[YRT_SLOT(sp)] = (e);                                                    \
    sp += 1;                                                                      \
  } while (0)
#define YRT_POP()                                                                 \
  do {                                                                            \
    if (sp == 0) {                                                                \
      curCnt = -1;                                                                \
    } else {                                                                      \
      sp -= 1;                                                                    \
      unsigned e_;                                                                \
      YRT_POP_READ(e_);                                                           \
      curIdx = (int)(e_ >> 5);                                                    \
      curCnt = (int)(e_ & 31u);                                                   \
    }                                                                             \
  } while (0)
  // ray kept as plain vectors across iterations (a loop-carried RayPre struct ends up in
  // scratch: the vectorizer's straddling loads defeat SROA); rebuilt in registers per step
  float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro, ri = ro, rc = ro;
  float rtime = 0.f;
  Hit best;
  best.t = best.u = best.v = 0.f;
  best.tri = -1;
  // closest hit: the accepted triangle's undivided barycentrics (U, V) and |den| are kept, and
  // u = U/|den|, v = V/|den| are divided once, when the finished query is stored at the next
  // refill (or at the wave's end), instead of at every accepted hit; q = -1: nothing to store
  float bestDen = 1.f;
  q = -1;
  // PRIM: a finished camera ray (q = its path id) — a hit is appended with its ray and hit
  // record to the depth-0 queue segment of its path id's 64-group (one atomic per segment among
  // the storing lanes); a miss gets the environment's radiance, loaded from the render
  // parameters where it is stored (a value held in registers through the loop costs four of
  // them). The camera rays traced are counted after the loop, no counter is carried through it.
  auto prim_store = [&]() {
    const bool hitp = best.tri >= 0;
    if (!hitp) {
      const float* mL = pr.fv.rp->missL;
      pr.pathL[q] = make_float4(mL[0], mL[1], mL[2], mL[3]);
    }
    const int seg = qseg_of((unsigned)q);
    unsigned long long m = ballot(hitp);
    while (m) {
      const int l0 = __ffsll((long long)m) - 1;
      const int seg0 = __builtin_amdgcn_readlane(seg, l0);
      const unsigned long long sub = ballot(hitp && seg == seg0);
      unsigned base = 0;
      if (lane == l0) base = atomicAdd(pr.counts + (size_t)seg0 * YRT_QCSTRIDE, (unsigned)__popcll(sub));
      base = (unsigned)__builtin_amdgcn_readlane((int)base, l0);
      if (hitp && seg == seg0) {
        const unsigned slot = (unsigned)seg0 * (unsigned)pr.segCap + base + lanes_below(sub);
        pr.qPath[slot] = q;
        pr.qOrg[slot] = ro;
        pr.qDir[slot] = rd;
        hitOut[slot] = make_float4(best.t, best.u / bestDen, best.v / bestDen, __int_as_float(best.tri));
      }
      m &= ~sub;
    }
  };
#define YRT_STORE_HIT()                                                                              \
  do {                                                                                               \
    if constexpr (PRIM)                                                                              \
      prim_store();                                                                                  \
    else                                                                                             \
      hitOut[q] = make_float4(best.t, best.u / bestDen, best.v / bestDen, __int_as_float(best.tri)); \
    q = -1;                                                                                          \
  } while (0)
  // a refilled lane's traversal state from its ray (ro, rd); NaN tfar (tMaxShadowRay = inf,
  // SURVEY App. A Q4): no hit, nothing to traverse
#define YRT_RAY_SETUP()                                                                   \
  do {                                                                                    \
    ri = make_float4(safe_inv(rd.x), safe_inv(rd.y), safe_inv(rd.z), 0.f);                \
    ri.w = __int_as_float(plane_offsets(ri.x, ri.y, ri.z));                               \
    {                                                                                     \
      V3 oi;                                                                              \
      float mg;                                                                           \
      ray_slab_consts(v3(ro.x, ro.y, ro.z), v3(ri.x, ri.y, ri.z), oi, mg);                \
      rc = make_float4(oi.x, oi.y, oi.z, mg);                                             \
    }                                                                                     \
    best.t = rd.w;                                                                        \
    best.u = best.v = 0.f;                                                                \
    best.tri = -1;                                                                        \
    bestDen = 1.f;                                                                        \
    sp = 0;                                                                               \
    curIdx = 0;                                                                           \
    curCnt = 0;                                                                           \
    pendCnt = 0;                                                                          \
    has = rd.w >= ro.w;                                                                   \
    if (!has) {                                                                           \
      if (ANY) shadow_done(sf, occOut, q, false);                                         \
    }                                                                                     \
  } while (0)

#ifdef YRT_PROFILE
  unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  while (true) {
    // retire lanes whose traversal is complete
    if (has && curCnt < 0 && pendCnt == 0) {
      if (ANY) shadow_done(sf, occOut, q, false);
      has = false;
    }
    const unsigned long long idle = ballot(!has);
    const int nIdle = __popcll(idle);
    YRT_PROF(0, 1);
    YRT_PROF(1, 64 - nIdle);
    if (nIdle >= (ANY ? YRT_REFILL_ANY : PRIM ? YRT_REFILL_PRIM : YRT_REFILL)) {
      if (next < end) {
        const unsigned li = next + lanes_below(idle);
        if (!has) {
          if constexpr (ANY) {
            // Fused: the pending lanes (q >= 0, see shadow_done) are resolved here. Their
            // contributions are loaded beside the new rays (one wait for both), their paths'
            // radiance before the new rays' setup arithmetic, which covers part of that second
            // round trip; the sum is stored last. The same l + c per channel as
            // k_shadow_resolve, one writer per path and launch.
            const bool resolve = sf.contrib && q >= 0;
            const bool take = li < end;
            // read under `resolve` only; set here all the same: left unset, the kernel spills
            // (44 B of scratch at 64 VGPRs)
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f), l = c;
            float4* Lp = nullptr;
            if (resolve) c = sf.contrib[q];
            q = -1;
            if (take) {
              q = qmap_phys(qm, segCap, li);
              ro = org[q];
              rd = dir[q];
              if (MOTION) rtime = rayTime[q];
            }
            // One wait for the contributions and the rays, here and on every path: the path id
            // and tfar are pinned as first used at this point. Without the pins the path id's
            // address arithmetic, and its wait with it, moves up to the contribution's load, and
            // the rays' wait into the setup below, behind the radiance's load.
            int tg = __float_as_int(c.w);
            asm volatile("" : "+v"(tg), "+v"(rd.w));
            if (resolve) {
              Lp = sf.pathL + tg;
              l = *Lp;
            }
            if (take) {
              // a ray with nothing to traverse and not fused: its flag is stored at once;
              // fused, it is pending like any unoccluded ray (has = false, q kept)
              YRT_RAY_SETUP();
            }
            asm volatile("" : "+v"(l.x));  // the radiance's wait, on every path too
            if (resolve) *Lp = make_float4(l.x + c.x, l.y + c.y, l.z + c.z, l.w);
          } else {
          if (!ANY && q >= 0) YRT_STORE_HIT();
          if (li < end) {
            if constexpr (PRIM) {
              // k_raygen's camera ray of path li (same operations, bit-identical rays)
              const YRT_CONST GpuRenderParams& rp = const_ref(pr.fv.rp);
              const int p = (int)li;
              const int smp = fastdiv(p, pr.bi.divPixels);
              int x = 0, y = 0, f = 0;
              const bool valid = batch_pixel(rp, pr.bi, p - smp * pr.bi.numPixels, x, y, f) && rp.maxDepth > 0 &&
                                 !(1.0f < rp.minContribution);
              if (valid) {
                const int rec = pr.fv.pixelSets[(size_t)y * rp.width + x] * rp.spp + smp;
                const float fx = (float(x) + samp(pr.fv, 0, rec)) * rp.rcpWidth;
                const float fy = (float(y) + samp(pr.fv, 1, rec)) * rp.rcpHeight;
                const float lx = samp(pr.fv, 2, rec), ly = samp(pr.fv, 3, rec);
                V3 o3 = v3s(0.f), d3 = v3s(0.f);
                // one pass per frame among the refilled lanes (almost always one): the frame's
                // camera record is read with scalar loads, as in k_raygen
                for (bool todo = true; todo;) {
                  const int f0 = __builtin_amdgcn_readfirstlane(f);
                  if (f == f0) {
                    const YRT_CONST GpuCamera& cam = const_ref(pr.fv.cam + f0);
                    camera_ray<false>(cam, fx, fy, o3, d3, lx, ly);
                    todo = false;
                  }
                }
                ro = make_float4(o3.x, o3.y, o3.z, 0.f);
                rd = make_float4(d3.x, d3.y, d3.z, __int_as_float(0x7f800000));
                q = p;
              } else {
                // a zero made here: a constant zero vector is hoisted out of the loop and held in
                // four registers (spilled at a 5-wave register target)
                const float z = opaque_zero();
                pr.pathL[p] = make_float4(z, z, z, z);  // not a pixel of the image
                q = -1;
                ro = make_float4(0.f, 0.f, 0.f, 1.f);  // tfar < tnear: nothing to traverse
                rd = make_float4(0.f, 0.f, 1.f, 0.f);
              }
            } else {
            q = qmap_phys(qm, segCap, li);
            ro = org[q];
            rd = dir[q];
            if (MOTION) rtime = rayTime[q];
            }
            YRT_RAY_SETUP();
          }
          }
        }
        next += (unsigned)nIdle;
      } else if (nIdle == 64) {
        if (!ANY && q >= 0) YRT_STORE_HIT();
        if constexpr (ANY) {
          // the lanes still pending when the chunk is used up
          if (sf.contrib && q >= 0) {
            const float4 c = sf.contrib[q];
            float4* Lp = sf.pathL + __float_as_int(c.w);
            const float4 l = *Lp;
            *Lp = make_float4(l.x + c.x, l.y + c.y, l.z + c.z, l.w);
          }
        }
        if constexpr (PRIM) {
          // the camera rays this wave traced: the valid path ids of its chunk (the refill's
          // test again, after the loop, so that no count is carried through it)
          const YRT_CONST GpuRenderParams& rp = const_ref(pr.fv.rp);
          unsigned t = 0;
          if (rp.maxDepth > 0 && !(1.0f < rp.minContribution)) {
            for (unsigned b = gw * chunk; b < end; b += 64) {
              const unsigned p = b + (unsigned)lane;
              bool v = false;
              if (p < end) {
                const int smp = fastdiv((int)p, pr.bi.divPixels);
                int x, y, f;
                v = batch_pixel(rp, pr.bi, (int)p - smp * pr.bi.numPixels, x, y, f);
              }
              t += (unsigned)__popcll(ballot(v));
            }
          }
          if (lane == 0 && t) atomicAdd(pr.traced, t);
        }
#ifdef YRT_PROFILE
        if (lane == 0)
          for (int k = 0; k < 8; ++k) atomicAdd(&g_traceProfile[k], prof[k]);
#endif
        break;
      }
    }
    RayPre r;
    r.org = v3(ro.x, ro.y, ro.z);
    r.dir = v3(rd.x, rd.y, rd.z);
    r.inv = v3(ri.x, ri.y, ri.z);
    r.tnear = ro.w;
    r.tfar = rd.w;
    r.oi = v3(rc.x, rc.y, rc.z);
    r.margin = rc.w;

    // One step per iteration, chosen wave-uniformly ("while-while" with speculative leaf
    // parking, Aila & Laine 2009): node steps while any lane still searches for its first
    // leaf (a lane reaching a leaf parks it and keeps descending), then one leaf step in
    // which every lane tests one leaf. Refill above runs every iteration, so lanes that
    // finish rejoin at once instead of idling until the wave's phase ends.
    // node step when more lanes can descend than are blocked on a leaf (cur is a leaf while
    // another is parked, or only a parked leaf is left); otherwise a leaf step
    // lane masks of plain comparisons (one v_cmp each) combined on the scalar unit: a ballot of
    // has && ... re-materializes the predicate per ballot (8 -> 3 VALU per node-step check,
    // closest-hit trace -2.1 % on C3, profiles/r02/trace_variants_r02.txt); has does not change
    // inside the node loop, so its mask is taken once here
    const unsigned long long hasB = ballot(has);
#define YRT_NNODE() __popcll(ballot(curCnt == 0) & hasB)
#define YRT_NBLOCKED() __popcll(ballot(max(pendCnt, curCnt) > 0) & ~ballot(curCnt == 0) & hasB)
    const int nNode = YRT_NNODE();
    const int nBlocked = YRT_NBLOCKED();
    if (nNode * 4 > nBlocked * (ANY ? YRT_NODE_BIAS_ANY : YRT_NODE_BIAS)) {
     // consecutive node steps without the retire/refill block in between (+1.5 % on C3)
     while (true) {
      YRT_PROF(2, 1);
      YRT_PROF(3, __popcll(ballot(has && curCnt == 0)));
      if (has && curCnt == 0) {
        float t[4];
        int c[4];
        // sign-ordered slab planes (+1.5 % on C3 with two lanes, bit-identical distances)
        box4_quant<ANY>(r, __float_as_int(ri.w), best.t, t, c, qnodes, curIdx);
        // closest-hit rays sort the hit children by entry distance (nearest next, the others
        // pushed farthest-first); any-hit rays take the farthest hit child next and push the
        // others in slot order (sort3_far: -22 % node visits against slot order)
        if (!ANY) sort4(t, c);
        else sort3_far(t, c);
        const float MISS = __int_as_float(ANY ? 0xff800000 : 0x7f800000);
#define YRT_HIT(x) (ANY ? (x) > MISS : (x) < MISS)
        if (sp + 3 <= kLds) {
          // all three candidates fit in free ring slots: store unconditionally, advance sp
          // only past the hit ones (a store of a missed child lands on a free slot);
          // shadow rays -4..9 %, closest neutral (profiles/r01)
          const int h3 = YRT_HIT(t[3]), h2 = YRT_HIT(t[2]), h1 = YRT_HIT(t[1]);
          stack[YRT_SLOT(sp)] = c[3];
          stack[YRT_SLOT(sp + h3)] = c[2];
          stack[YRT_SLOT(sp + h3 + h2)] = c[1];
          sp += h3 + h2 + h1;
        } else {
          if (YRT_HIT(t[3])) YRT_PUSH(c[3]);
          if (YRT_HIT(t[2])) YRT_PUSH(c[2]);
          if (YRT_HIT(t[1])) YRT_PUSH(c[1]);
        }
        if (YRT_HIT(t[0])) {
          curIdx = c[0] >> 5;
          curCnt = c[0] & 31;
        } else {
          YRT_POP();
        }
#undef YRT_HIT
        if (curCnt > 0 && pendCnt == 0) {
          pendIdx = curIdx;
          pendCnt = curCnt;
          YRT_POP();
        }
      }
      const int nNode2 = YRT_NNODE();
      const int nBlocked2 = YRT_NBLOCKED();
      if (!(nNode2 * 4 > nBlocked2 * (ANY ? YRT_NODE_BIAS_ANY : YRT_NODE_BIAS))) break;
     }
    } else {
      // leaf step: the parked leaf, or else the current entry when it is a leaf
      const bool usePend = pendCnt > 0;
      const int lIdx = usePend ? pendIdx : curIdx;
      const int lCnt = !has ? 0 : usePend ? pendCnt : (curCnt > 0 ? curCnt : 0);
#ifdef YRT_PROFILE
      {
        const int lc_ = min(lCnt, ANY ? YRT_TRI_STEP_ANY : kTriStep);  // triangles this step
        int mx = lc_;
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        int sm = lc_;
        for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
        YRT_PROF(4, mx > 0 ? 1 : 0);
        YRT_PROF(5, mx);
        YRT_PROF(6, sm);
      }
#endif
      bool found = false;
      // at most kTriStep (YRT_TRI_STEP_ANY) triangles per lane per leaf step (the rest of
      // the leaf stays current / parked): less intra-leaf divergence
      const int lTake = min(lCnt, ANY ? YRT_TRI_STEP_ANY : kTriStep);
      if (!ANY) {
        // closest hit: all triangles of the step loaded up front (one memory round trip instead
        // of one per triangle: closest trace -4.6 % on C3, profiles/r02/trace_variants_r02.txt),
        // then accepted in leaf order; lanes with fewer triangles repeat their last one and
        // ignore it
        if (lTake > 0) {
          GpuTri tt[kTriStep];
#pragma unroll
          for (int k = 0; k < kTriStep; ++k) tt[k] = tri_at<MOTION>(tris, sv.triMotion, lIdx + min(k, lTake - 1), rtime);
#pragma unroll
          for (int k = 0; k < kTriStep; ++k) {
            float t, U, V, absDen;
            const bool g = tri_test_g(tt[k], r, t, U, V, absDen);
            const int gid = __float_as_int(tt[k].v0[3]);
            // range test against the current closest hit; on a tie (t == best.t) the smaller
            // triangle id wins
            // a tie with an accepted hit (best.tri >= 0, so best.t < tfar) passes the range test
            // by itself: one predicate instead of a re-test against tfar (C3 -0.35 %, C5 -0.3 %).
            // The same rule as closest_hit (yrt_traverse.h), inline here: a shared helper
            // re-allocates this kernel's registers.
            const bool tie = (t == best.t) & (best.tri >= 0) & (gid < best.tri);
            const bool ok = g & (t > r.tnear) & ((t < best.t + 0.0f) | tie);
            if (ok & (k < lTake)) {
              best.t = t; best.u = U; best.v = V; bestDen = absDen; best.tri = gid;
            }
          }
        }
      } else {
        // any hit: one triangle after the other, until the first hit
        for (int i = 0; i < lTake && !found; ++i) {
          const GpuTri tr = tri_at<MOTION>(tris, sv.triMotion, lIdx + i, rtime);
          float t, U, V, absDen;
          found = tri_test_t(tr, r, r.tfar, t, U, V, absDen);
        }
      }
      if (lCnt > 0) {
        if (usePend) {
          pendIdx += lTake;
          pendCnt -= lTake;
        } else if (curCnt > lTake) {
          curIdx += lTake;
          curCnt -= lTake;
        } else {
          YRT_POP();
        }
      }
      if (ANY && found) {
        shadow_done(sf, occOut, q, true);
        has = false;
      }
    }
  }
}

#undef YRT_SLOT
#undef YRT_POP_READ
#undef YRT_PUSH
#undef YRT_POP
#undef YRT_STORE_HIT
#undef YRT_RAY_SETUP
#undef YRT_NNODE
#undef YRT_NBLOCKED
#undef YRT_PROF

}  // namespace yrt
