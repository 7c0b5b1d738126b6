// render_job.cpp — the batch plan and the wavefront lane scheduler of one shard's render
// (render_job.h). Reference counterpart: IntegratorRenderer::RenderJob
// (renderers/integratorrenderer.cpp:63-185), whose tile loop the batches restate.
#include "render_job.h"

namespace yrt {

RenderSwitches RenderSwitches::read() {
  RenderSwitches sw;
  sw.primary = getenv("YRT_PRIMARY") ? atoi(getenv("YRT_PRIMARY")) : 1;
  sw.primaryMiss = getenv("YRT_PRIMARY_MISS") ? atof(getenv("YRT_PRIMARY_MISS")) : 0.5;
  sw.noShadowFuse = getenv("YRT_NO_SHADOW_FUSE") != nullptr;
  sw.allDirectLights = getenv("YRT_ALL_DIRECT_LIGHTS") != nullptr;
  sw.batchGrow = !(getenv("YRT_BATCH_GROW") && atoi(getenv("YRT_BATCH_GROW")) == 0);
  return sw;
}

BatchPlan plan_batches(int64_t shardTiles, int spp, int64_t capacity, int numLanes, bool capture, bool grow) {
  int64_t tilesPerBatch = std::max<int64_t>(1, capacity / (256ll * spp));
  // a multiple of the lanes in batches (evenly sized), so both lanes have work even when a
  // shard of the frame fits one batch (multi-GPU shards, small frames)
  if (!capture && numLanes > 1 && shardTiles > 1) {
    int64_t nb = (shardTiles + tilesPerBatch - 1) / tilesPerBatch;
    nb = (nb + numLanes - 1) / numLanes * numLanes;
    // At the default capacity, a lane that would run 5-8 batches runs half as many of twice
    // the size: each batch pays a fixed chain of 10 depths x 3 launches and a ramp-down, which
    // outweighs the overlap the extra batches buy there (C4 N = 8 rank share 51.0 -> 48.7 ms;
    // at 27+ batches per lane, N = 1 / 2, twice the size measured +1 / +4 %,
    // profiles/r04/ab_r04k.txt, scaling_prediction_c4_r04z.txt). YRT_BATCH_GROW=0: off.
    grow = grow && capacity == ((int64_t)YRT_DEFAULT_CAPACITY_M << 20);
    if (grow && nb > 4 * numLanes && nb <= 8 * numLanes) {
      nb = (nb / 2 + numLanes - 1) / numLanes * numLanes;
    } else if (grow && nb > 8 * numLanes && nb <= 16 * numLanes) {
      // 9-16 per lane: 1.5x the size (C4 N = 4 share, 96 M paths: 100 -> 95 ms, ab_r04k.txt)
      nb = (nb * 2 / 3 + numLanes - 1) / numLanes * numLanes;
    }
    tilesPerBatch = (shardTiles + nb - 1) / nb;
  }
  BatchPlan p;
  p.tilesPerBatch = tilesPerBatch;
  p.pathsPerBatch = std::min<int64_t>(tilesPerBatch, shardTiles) * 256 * spp;
  p.numBatches = (shardTiles + tilesPerBatch - 1) / tilesPerBatch;
  // the capture frame (roofline accounting) reads batch 0's queues synchronously: one lane
  p.lanes = capture ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(numLanes, p.numBatches));
  return p;
}

ShardJob::ShardJob(const Device& D, GpuCtx& g, const GpuScene& G, RendererObj& R, const ShardSetup& s,
                   const BatchPlan& plan)
    : g(g), G(G), R(R), s(s), plan(plan), kernelTiming(D.kernelTiming), captureMax(D.captureMax),
      levels(s.rp.maxDepth + 1), counterWords(qcounter_words(levels) + 1), tracedWord(counterWords - 1),
      numDirect(s.sv.numDirectLights), jobs(plan.lanes) {}

// the lanes' streams, queues and counter read-back slots, sized for the plan's batches
void ShardJob::prepare_lanes() {
  const GpuRenderParams& rp = s.rp;
  const int nl = plan.lanes;
  g.ensure_streams(nl);
  for (int l = 0; l < nl; ++l) {
    Lane& L = g.lanes[l];
    GpuCtx::ensure_paths(L, std::max<int64_t>(plan.pathsPerBatch, 256ll * rp.spp), numDirect, G.hasMotion);
    L.counters.alloc(counterWords * sizeof(unsigned));
    L.spill.alloc(YRT_TRACE_SPILL_INTS * sizeof(int));
    for (Lane::Pend& Pd : L.pend) {
      if (Pd.hcWords < counterWords) {
        if (Pd.hc) HIP_CHECK(hipHostFree(Pd.hc));
        Pd.hc = nullptr;
        Pd.hcWords = 0;
        HIP_CHECK(hipHostMalloc((void**)&Pd.hc, counterWords * sizeof(unsigned), hipHostMallocDefault));
        Pd.hcWords = counterWords;
      }
      if (!Pd.done) HIP_CHECK(hipEventCreateWithFlags(&Pd.done, hipEventDisableTiming));
    }
    L.pendHead = L.pendCount = 0;
    jobs[l].pb = lane_buffers(L);
    jobs[l].sv = s.sv;
    jobs[l].sv.traceSpill = L.spill.as<int>();
  }
  // the other lanes start after the frame setup enqueued on lane 0 (uploads, pixel sets)
  if (nl > 1) {
    hipEvent_t setup = g.ev();
    HIP_CHECK(hipEventRecord(setup, g.stream));
    for (int l = 1; l < nl; ++l) HIP_CHECK(hipStreamWaitEvent(g.lanes[l].stream, setup, 0));
  }
}

PathBuffers ShardJob::lane_buffers(Lane& L) const {
  PathBuffers pb;
  for (int k = 0; k < 2; ++k) {
    pb.qPath[k] = L.qPath[k].as<int>();
    pb.qOrg[k] = L.qOrg[k].as<float4>();
    pb.qDir[k] = L.qDir[k].as<float4>();
    pb.qThr[k] = L.qThr[k].as<float4>();
  }
  pb.hit = L.hit.as<float4>();
  pb.pathL = L.pathL.as<float4>();
  pb.shFirst = L.shFirst.as<int>();
  pb.sOrg = L.sOrg.as<float4>();
  pb.sDir = L.sDir.as<float4>();
  pb.sContrib = L.sContrib.as<float4>();
  pb.sOcc = L.sOcc.as<int>();
  pb.counters = L.counters.as<unsigned>();
  for (int k = 0; k < 2; ++k) pb.qTime[k] = G.hasMotion ? L.qTime[k].as<float>() : nullptr;
  pb.sTime = G.hasMotion ? L.sTime.as<float>() : nullptr;
  pb.capacity = (int)std::max<int64_t>(plan.pathsPerBatch, 256ll * s.rp.spp);
  pb.segCap = qseg_capacity(pb.capacity);
  pb.shSegCap = pb.segCap * std::max(1, numDirect);
  // one light: shadow contributions are added by k_trace<true> itself (no resolve pass)
  pb.fuseShadow = numDirect == 1 && !s.sw.noShadowFuse;
  pb.reserved = const_cast<int*>(s.tileList);  // list mode of batch_tile (kernels/yrt_camera.h)
  return pb;
}

// accounts the queue counters of the lane's oldest pending batch; without `wait` only if
// the batch's counters have arrived (returns whether it accounted one)
bool ShardJob::drain_one(Lane& L, bool wait) {
  if (L.pendCount == 0) return false;
  Lane::Pend& Pd = L.pend[L.pendHead];
  if (wait) {
    HIP_CHECK(hipEventSynchronize(Pd.done));
  } else {
    const hipError_t q = hipEventQuery(Pd.done);
    if (q == hipErrorNotReady) return false;
    HIP_CHECK(q);
  }
  const int maxDepth = s.rp.maxDepth;
  for (int d = 0; d < levels; ++d) {
    double nc = 0, ns = 0;
    for (int k = 0; k < YRT_QSEGS; ++k) {
      nc += Pd.hc[qcounter_index(d, 0, k)];
      ns += Pd.hc[qcounter_index(d, 1, k)];
    }
    if (d == 0 && Pd.fused && Pd.hc[tracedWord] > 0) {
      if (g.missFrac.size() > 64 && !g.missFrac.count(G.serial)) g.missFrac.clear();
      auto& acc = g.missFrac[G.serial];
      acc.first += (double)Pd.hc[tracedWord] - nc;  // a fused depth 0 queues its hits only
      acc.second += (double)Pd.hc[tracedWord];
      missEst = acc.first / acc.second;
    }
    if (d < maxDepth) {  // level maxDepth counts continuations that are never traced
      // a fused depth 0 queues its hits only: the camera rays it traced are counted apart
      const double traced = d == 0 && Pd.fused ? (double)Pd.hc[tracedWord] : nc;
      g.stats.raysClosest += traced;
      if (traced) g.stats.launchesClosest += 1;
    }
    g.stats.raysShadow += ns;
    if (d < maxDepth && ns) g.stats.launchesShadow += 1;
  }
  L.pendHead = (L.pendHead + 1) % Lane::kPendDepth;
  L.pendCount -= 1;
  tilesDone += Pd.tiles;
  if (s.reportProgress) status(R, 1, float(tilesDone) / float(std::max(1, s.shardTiles)));
  return true;
}

// gives every lane that holds no batch (and whose previous batch's counters have arrived) the
// shard's next batch
void ShardJob::start_batches() {
  for (int l = 0; l < plan.lanes && nextFirst < s.shardTiles; ++l) {
    LaneJob& J = jobs[l];
    if (J.active || g.lanes[l].pendCount >= Lane::kPendDepth) continue;
    J.active = true;
    J.step = 0;
    J.seq = batch++;
    const int64_t batchTiles = std::min<int64_t>(plan.tilesPerBatch, s.shardTiles - nextFirst);
    J.first = nextFirst;
    J.bi.firstTile = (int)nextFirst;
    // a listed batch names its tiles itself: the arithmetic members stay the identity
    J.bi.tileStride = s.tileList ? 1 : s.count;
    J.bi.tileOffset = s.tileList ? 0 : s.index;
    nextFirst += batchTiles;
    J.bi.numPixels = (int)(batchTiles * 256);
    J.bi.divPixels = fastdiv_make((uint32_t)J.bi.numPixels);
    // fused (hits queued) while camera rays mostly miss, k_raygen + the queued trace otherwise
    J.fused = fusedPrimary &&
              (s.sw.primary == 2 || (s.sw.primary == 1 && (missEst < 0 || missEst >= s.sw.primaryMiss)));
  }
}

// yrtSetKernelTiming: the launch's HIP-event time goes to `sum` of the GPU's render stats
template <class Launch>
void ShardJob::timed(double YRTRenderStats::*sum, hipStream_t st, Launch&& launch) {
  EvPair ev;
  ev.time(kernelTiming, st, launch);
  if (ev.b) evs.push_back(Timed{std::move(ev), sum});
}

// enqueues the next step of the lane's batch on the lane's stream
void ShardJob::enqueue_step(Lane& L, LaneJob& J) {
  const hipStream_t st = L.stream;
  const PathBuffers& pb = J.pb;
  const FrameView& fv = s.fv;
  const BatchInfo& bi = J.bi;
  const int maxDepth = s.rp.maxDepth;
  if (J.step == 0) {
    HIP_CHECK(hipMemsetAsync(L.counters.p, 0, counterWords * sizeof(unsigned), st));
    if (!J.fused) launch_raygen(fv, pb, bi, st);
  } else if (J.step <= maxDepth) {
    const int d = J.step - 1;
    const int cur = d & 1;
    timed(&YRTRenderStats::msTraceClosest, st, [&] {
      if (d == 0 && J.fused) {
        PrimaryRays pr;
        pr.fv = fv;
        pr.bi = bi;
        pr.qPath = pb.qPath[0];
        pr.qOrg = pb.qOrg[0];
        pr.qDir = pb.qDir[0];
        pr.pathL = pb.pathL;
        pr.counts = pb.counters + qcounter_index(0, 0, 0);
        pr.segCap = pb.segCap;
        pr.traced = pb.counters + tracedWord;
        pr.numPaths = (long long)bi.numPixels * s.rp.spp;
        launch_trace_primary(J.sv, pr, pb.hit, st);
      } else {
        launch_trace_closest(J.sv, pb.qOrg[cur], pb.qDir[cur], pb.counters + qcounter_index(d, 0, 0), YRT_QSEGS,
                             pb.segCap, pb.hit, st, pb.qTime[cur]);
      }
    });
    if (captureMax > 0 && J.first == 0)
      g.capture(captureMax, g.capClosest, d, pb.qOrg[cur], pb.qDir[cur], pb.counters + qcounter_index(d, 0, 0),
                pb.segCap, st);
    timed(&YRTRenderStats::msShade, st, [&] { launch_shade(J.sv, fv, pb, bi, d, G.materialMask, st); });
    if (numDirect > 0) {
      timed(&YRTRenderStats::msTraceShadow, st, [&] {
        const ShadowFuse sf{pb.fuseShadow ? pb.sContrib : nullptr, pb.pathL};
        launch_trace_any(J.sv, pb.sOrg, pb.sDir, pb.counters + qcounter_index(d, 1, 0), YRT_QSEGS, pb.shSegCap,
                         pb.sOcc, st, &sf, pb.sTime);
      });
      if (captureMax > 0 && J.first == 0)
        g.capture(captureMax, g.capShadow, d, pb.sOrg, pb.sDir, pb.counters + qcounter_index(d, 1, 0),
                  pb.shSegCap, st);
      if (!pb.fuseShadow) launch_shadow_resolve(pb, d, numDirect, st);
    }
  } else {
    // the counters are final after the last trace: their copy runs before the pixel resolve,
    // so the host learns the batch's queue sizes while the resolve still runs
    Lane::Pend& Pd = L.pend[(L.pendHead + L.pendCount) % Lane::kPendDepth];
    HIP_CHECK(hipMemcpyAsync(Pd.hc, L.counters.p, counterWords * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(Pd.done, st));
    Pd.tiles = bi.numPixels / 256;
    Pd.fused = J.fused;
    Pd.seq = J.seq;
    L.pendCount += 1;
    launch_resolve_pixels(fv, pb, bi, g.fbFloat(), g.fbRGB8(), (int)rgb8_row_stride(s.rp.width),
                          g.accu, s.accumulate ? 1 : 0, st);
    // an even iteration of an adaptive render: the same batch added into the half buffer, no display
    if (s.half) launch_resolve_pixels(fv, pb, bi, nullptr, nullptr, 0, s.half, 1, st);
    J.active = false;
  }
  J.step += 1;
}

void ShardJob::run() {
  g.capClosest.clear();
  g.capShadow.clear();
  prepare_lanes();
  const int nl = plan.lanes;
  auto mit = g.missFrac.find(G.serial);
  missEst = mit == g.missFrac.end() ? -1.0 : mit->second.first / mit->second.second;
  // Depth 0 as one kernel (launch_trace_primary): camera rays generated inside the closest-hit
  // trace, misses resolved there, only hits queued for k_shade — for static scenes whose
  // depth-0 miss radiance is a constant: no backplate, every environment light ambient
  // (k_shade's miss branch then adds thr * L = L per light in envLights order, thr = 1).
  // Not in the capture frame (it copies the depth-0 queue). It pays where camera rays miss
  // (C4: cube job -11 %, -1.3 % more at 96 VGPRs / 5 waves since round 5) and costs where they
  // hit (C3 -2.5 %, C5 -1.3 %: its hits are appended in completion order, profiles/r04/
  // ab_r04d.txt; a path-ordered "identity" layout measured no better, profiles/r05/
  // ab_prim_r05j.txt), so a batch is fused while the scene's measured miss share (missFrac, over
  // its fused batches so far) is at least YRT_PRIMARY_MISS (default 0.5) or unknown.
  // YRT_PRIMARY=0: never, 2: always.
  // Toe-in stereo cameras (the DLL's FPR default) are left to k_raygen: the fused kernel is
  // compiled without that branch (camera_ray<false>, kernels/yrt_camera.h).
  bool toeIn = false;
  for (const GpuCamera& c : g.hCams) toeIn |= c.type == CAM_STEREO && c.toeIn != 0;
  fusedPrimary = captureMax == 0 && !G.hasMotion && !s.fv.backplateTexels && s.sv.numEnvDir == 0 &&
                 s.sw.primary != 0 && !toeIn && !s.tileList;  // PrimaryRays carries no tile list
  // A lane's batch is enqueued a step at a time — its prologue (counter clear, camera rays),
  // one depth (closest trace, shade, shadow trace), its epilogue (counter copy, pixel resolve)
  // — round-robin over the lanes that hold a batch, so every lane's first kernels are queued
  // within a few launches of the job's start. A whole batch at a time (≈ 33 launches at
  // ≈ 58 µs of host time each), lane k started k × 1.9 ms after lane 0 and the job's end waited
  // as long for the last lane (C3 N = 8 share: lanes starting 0 / 1.1 / 3.1 / 5.1 ms into a
  // 52.7 ms job, profiles/r05/timeline_c3_n8_r05v.txt). A lane takes its next batch once its
  // previous batch's counters have arrived (Pend); the batch goes to the first such lane, so a
  // lane that finishes early is refilled at once (lanes in turn: C4 N = 3 rank share 160 ms,
  // profiles/r04/ab_r04i.txt). When every lane is full the host blocks on the batch enqueued
  // first (hipEventSynchronize) instead of spinning a core.
  for (;;) {
    if (R.stopFlag && R.stopFlag->load()) nextFirst = s.shardTiles;  // no new batches
    for (int l = 0; l < nl; ++l)
      while (drain_one(g.lanes[l], false)) {}
    start_batches();
    bool enqueued = false;
    for (int l = 0; l < nl; ++l)
      if (jobs[l].active) {
        enqueue_step(g.lanes[l], jobs[l]);
        enqueued = true;
      }
    if (enqueued) continue;
    if (nextFirst >= s.shardTiles) break;  // every batch enqueued
    // every lane holds a batch whose counters have not arrived: wait for the oldest
    int oldest = 0;
    for (int l = 1; l < nl; ++l)
      if (g.lanes[l].pend[g.lanes[l].pendHead].seq < g.lanes[oldest].pend[g.lanes[oldest].pendHead].seq) oldest = l;
    drain_one(g.lanes[oldest], true);
  }
  for (int l = 0; l < nl; ++l)
    while (drain_one(g.lanes[l], true)) {}
  for (Timed& e : evs) {
    float ms = 0;
    e.ev.read(ms);
    g.stats.*e.sum += ms;
  }
  evs.clear();
  for (auto e : g.eventPool) (void)hipEventDestroy(e);
  g.eventPool.clear();
}

}  // namespace yrt
