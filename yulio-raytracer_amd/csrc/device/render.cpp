// render.cpp — the frame job of the device plugin: Device::render deals a job's tiles over the
// process's GPUs, gathers them and hands the frames to their framebuffers; Device::render_shard
// sets one GPU's share up and runs it as a wavefront job (render_job.h).
//
// Reference counterparts: IntegratorRenderer::renderFrame (renderers/integratorrenderer.cpp:63-185),
// DebugRenderer (renderers/debugrenderer.cpp:66-140).
#include <chrono>
#include <thread>

#include "device.h"
#include "render_job.h"

namespace yrt {

// Frames of an earlier job not yet read back: this job renders into another block. With
// blk and spareBlk both holding unread frames a new block is allocated, up to
// kMaxFrameBlocks alive; past that the block about to be reused is read back into its
// framebuffers' host pixels first (rtMapFrameBuffer then finds them there), so frames
// nobody maps cannot pin HBM without bound
void Device::rotate_frame_block() {
  GpuCtx& g0 = *ctx[0];
  if (g0.blk.use_count() > 1) {
    std::swap(g0.blk, g0.spareBlk);
    if (!g0.blk || g0.blk.use_count() > 1) {
      auto& xb = g0.extraBlocks;
      xb.erase(std::remove_if(xb.begin(), xb.end(), [](const std::weak_ptr<GpuCtx::FrameBlock>& w) {
                 return w.expired();
               }), xb.end());
      // blocks alive: blk, spareBlk and the extra ones (spareBlk is usually one of those)
      int live = (g0.blk ? 1 : 0) + (g0.spareBlk ? 1 : 0);
      for (const auto& w : xb) {
        const auto b = w.lock();
        live += b && b != g0.blk && b != g0.spareBlk;
      }
      if (g0.blk && live >= GpuCtx::kMaxFrameBlocks) {
        read_back_block(g0.blk.get());
      } else {
        g0.blk = std::make_shared<GpuCtx::FrameBlock>();
        xb.push_back(g0.blk);
      }
    }
  }
}

float4* Device::frame_accu(FrameBufferObj& F, GpuCtx& g) {
  for (const auto& a : F.accu)
    if (a->ctxSerial == g.serial) return a->sums.as<float4>();
  HIP_CHECK(hipSetDevice(g.hipDevice));
  auto a = std::make_unique<FrameBufferObj::Accu>();
  a->ctxSerial = g.serial;
  const size_t bytes = (size_t)F.width * F.height * sizeof(float4);
  a->sums.alloc(bytes);
  // AccuBuffer::clear (api/framebuffer.h:268-272) stores the weight 1e-10, which the first frame's
  // weight absorbs (1e-10 + spp == spp in float for spp >= 1): zeros give the same sums
  HIP_CHECK(hipMemsetAsync(a->sums.p, 0, bytes, g.stream));
  F.accu.push_back(std::move(a));
  return F.accu.back()->sums.as<float4>();
}

void Device::render(RendererObj& R, const std::vector<CameraObj*>& C, SceneObj& S, ToneMapperObj& T,
                    const std::vector<FrameBufferObj*>& F, int accumulate) {
  auto t0 = std::chrono::steady_clock::now();
  auto tRendered = t0;  // this process's tiles rendered (before any gather)
  // A process-level gather (yrtSetShardComm) is collective: every rank must reach it, so any
  // failure of this rank's part (arguments, scene, kernels) is reported to the peers through
  // the status exchange at its start instead of being thrown past it.
  const bool procGather = !R.debug && proc_gather_armed();
  const int nf = (int)F.size();
  const int W = nf ? F[0]->width : 0, H = nf ? F[0]->height : 0;
  const int tilesPerFrame = ((W + 15) / 16) * ((H + 15) / 16);
  const int numTiles = tilesPerFrame * nf;
  const bool rgb8 = nf && F[0]->format == FB_RGB8;
  SlabLayout base{W, H, (int)rgb8_row_stride(W), tilesPerFrame, 0, 1, rgb8 ? 1 : 0, 0};
  const int N = (int)ctx.size();
  // the debug renderer is a one-pass traversal KAT: the primary device renders every tile
  const int nr = R.debug ? 1 : N;
  std::string localErr;
  int gatherPath = YRT_GATHER_NONE;
  try {
    if (!S.gpu) throw std::runtime_error("scene not committed");
    if (S.gpu->device != hipDevice) throw std::runtime_error("scene committed on another HIP device");
    if (nf < 1 || (int)C.size() != nf) throw std::runtime_error("rtRenderFrames: one camera per framebuffer");
    for (const FrameBufferObj* f : F)
      if (f->width != W || f->height != H || f->format != F[0]->format)
        throw std::runtime_error("rtRenderFrames: framebuffers differ in size or format");
    if (R.debug && nf > 1) {
      // the debug renderer is a one-frame traversal KAT: its frames go one by one
      YRTRenderStats acc{};
      for (int k = 0; k < nf; ++k) {
        render(R, {C[k]}, S, T, {F[k]}, accumulate);
        acc.raysClosest += stats.raysClosest;
        acc.samples += stats.samples;
      }
      acc.msTotal = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      stats = acc;
      return;
    }
    memset(&stats, 0, sizeof(stats));
    // A multi-frame job resolves into a scratch block, not into its framebuffers' own sums, so
    // there is nothing of its frame for a later frame to be averaged with
    if (accumulate && nf == 1 && !R.debug && F[0]->accuFromJob)
      throw std::runtime_error("rtRenderFrame: accumulate=1 on a framebuffer whose last frame came from a multi-frame "
                               "job (rtRenderFrames keeps no accumulation): render it with accumulate=0 first");
    // an adaptive render leaves tiles of different iteration counts: no later frame continues them
    if (accumulate && nf == 1 && !R.debug && F[0]->accuFromAdaptive)
      throw std::runtime_error("rtRenderFrame: accumulate=1 on a framebuffer whose last frame came from an adaptive "
                               "render (rtRenderAdaptive stops tiles at different iterations): render it with "
                               "accumulate=0 first");
    if (!accumulate) R.iteration = 0;
    rotate_frame_block();
    std::vector<GpuScene*> scenes(nr);
    for (int k = 0; k < nr; ++k) scenes[k] = &scene_on(S, ctx[k]->hipDevice, k == 0);
    // the accumulation belongs to the framebuffer (found here, before the shards' threads start)
    std::vector<float4*> accu(nr, nullptr);
    if (nf == 1 && !R.debug)
      for (int k = 0; k < nr; ++k) accu[k] = frame_accu(*F[0], *ctx[k]);
    // Without a process gather, the pixels of the other processes' shards (yrtSetTileShard)
    // must read as zeros so per-process images compose by sum: ctx[0]'s block is cleared
    // outside the tiles this call writes. With several devices in the process and no
    // process-level shard (shardCount 1), the local gather writes every tile: no clear.
    shardZero = !procGather && (nr == 1 || shardCount > 1);
    if (nr == 1) {
      render_shard(*ctx[0], *scenes[0], R, C, T, W, H, shardIndex, shardCount, accumulate, true, accu[0]);
      tRendered = std::chrono::steady_clock::now();
    } else {
      // device k of this process renders the tiles t = shardIndex + k * shardCount (mod shardCount * N)
      std::vector<std::string> errs(nr);
      std::vector<std::thread> th;
      for (int k = 0; k < nr; ++k)
        th.emplace_back([&, k] {
          try {
            render_shard(*ctx[k], *scenes[k], R, C, T, W, H, shardIndex + k * shardCount, shardCount * nr,
                         accumulate, k == 0, accu[k]);
          } catch (const std::exception& e) {
            errs[k] = e.what();
          }
        });
      for (auto& t : th) t.join();
      for (auto& e : errs)
        if (!e.empty()) throw std::runtime_error(e);
      tRendered = std::chrono::steady_clock::now();
      gatherPath = gather_local(base, numTiles);
    }
  } catch (const std::exception& e) {
    if (!procGather) throw;
    localErr = e.what();
  }
  if (procGather) {
    gather_process(base, numTiles, localErr.empty(),
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    gatherPath = proc->kind()[0] == 'r' ? YRT_GATHER_RCCL_PROCESS : YRT_GATHER_HUB;
  }
  if (!localErr.empty()) throw std::runtime_error(localErr);
  R.iteration++;
  if (!R.debug)
    for (FrameBufferObj* f : F) {
      f->accuFromJob = nf > 1;
      f->accuFromAdaptive = false;
    }
  for (int k = 0; k < nr; ++k) {
    const YRTRenderStats& s = ctx[k]->stats;
    stats.raysClosest += s.raysClosest;
    stats.raysShadow += s.raysShadow;
    stats.launchesClosest += s.launchesClosest;
    stats.launchesShadow += s.launchesShadow;
    stats.msTraceClosest = std::max(stats.msTraceClosest, s.msTraceClosest);
    stats.msTraceShadow = std::max(stats.msTraceShadow, s.msTraceShadow);
    stats.msShade = std::max(stats.msShade, s.msShade);
  }

  // framebuffer write-back (api/framebuffer.h:93-226) from the primary device, frame by frame.
  // The other ranks of a process gather hold only their tiles: their host pixels are not
  // written (rank 0's framebuffers receive the gathered frames). A framebuffer with its own
  // host pixels keeps a reference to the frame in HBM instead, read back by rtMapFrameBuffer
  // (the reference's only access to the pixels, singleray_device.cpp:439-447): frames nobody
  // maps cross no PCIe.
  if (!(procGather && shardIndex != 0)) hand_over_frames(F, W, H);
  stats.samples = ctx[0]->stats.samples;
  stats.gather = gatherPath;
  const auto tEnd = std::chrono::steady_clock::now();
  if (tRendered == t0) tRendered = tEnd;  // the render threw before its end (collective error path)
  stats.msTotal = std::chrono::duration<double, std::milli>(tEnd - t0).count();
  stats.msRender = std::chrono::duration<double, std::milli>(tRendered - t0).count();
  stats.msGather = std::chrono::duration<double, std::milli>(tEnd - tRendered).count();
  status(R, 2, 1.f);
}

void Device::hand_over_frames(const std::vector<FrameBufferObj*>& F, int W, int H) {
  GpuCtx& g0 = *ctx[0];
  HIP_CHECK(hipSetDevice(g0.hipDevice));
  for (int k = 0; k < (int)F.size(); ++k) {
    FrameBufferObj& Fk = *F[k];
    FrameBufferObj::Pending pf;
    pf.keep = g0.blk;
    pf.src = Fk.format == FB_RGB8 ? (const void*)(g0.fbRGB8() + GpuCtx::FrameBlock::rgb8_bytes(W, H, k))
                                  : (const void*)(g0.fbFloat() + (size_t)k * W * H * 3);
    pf.hipDevice = g0.hipDevice;
    if ((int)Fk.pending.size() < Fk.depth) Fk.pending.resize(Fk.depth);
    Fk.pending[Fk.cur] = pf;
    if (!Fk.userPtrs.empty()) fb_read_back(Fk, Fk.cur);
  }
}

// samples: PathTraceIntegrator::requestSamples (pathtraceintegrator.cpp:35-47)
static SampleRequest sample_request(const RendererObj& R, const GpuScene& G) {
  SampleRequest req;
  req.spp = R.debug ? 1 : R.spp;
  req.sets = R.sets;
  req.iteration = R.iteration;
  req.num1D = R.debug ? 0 : R.maxDepth;
  req.num2D = R.debug ? 0 : 1 + R.maxDepth;
  req.filter = R.filter;
  if (!R.debug) req.lights = G.precomputed;
  return req;
}

// the frame's GpuRenderParams, but for spp and sets (the sample table's)
static GpuRenderParams render_params(const RendererObj& R, const ToneMapperObj& T, const GpuScene& G,
                                     const SampleRequest& req, int W, int H, int nf, uint32_t frameSeed) {
  GpuRenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.width = W;
  rp.height = H;
  rp.numTilesX = (W + 15) / 16;
  rp.numTilesY = (H + 15) / 16;
  rp.rcpWidth = rcpf_(float(W));
  rp.rcpHeight = rcpf_(float(H));
  rp.gamma = T.gamma;
  rp.rcpGamma = rcpf_(T.gamma);
  rp.vignetting = T.vignetting ? 1 : 0;
  rp.frameSeed = frameSeed;
  rp.maxDepth = R.maxDepth;
  rp.rrDepth = R.rrDepth;
  rp.minContribution = R.minContribution;
  rp.epsilon = R.epsilon;
  rp.tMaxShadowRay = R.tMaxShadowRay;
  rp.tMaxShadowJitter = R.tMaxShadowJitter;
  rp.up[0] = R.up.x; rp.up[1] = R.up.y; rp.up[2] = R.up.z;
  rp.numLights = G.view.numLights;
  rp.numEnvLights = G.view.numEnvLights;
  rp.numPrecomp = (int)G.precomputed.size();
  rp.numFrames = nf;
  rp.tilesPerFrame = rp.numTilesX * rp.numTilesY;
  rp.divTilesX = fastdiv_make((uint32_t)rp.numTilesX);
  rp.divTilesPerFrame = fastdiv_make((uint32_t)rp.tilesPerFrame);
  rp.dim1D = req.num1D;
  rp.dim2D = req.num2D;
  rp.lightSampleID = 0;
  rp.firstScatterSampleID = 1;
  rp.firstScatterTypeSampleID = 0;
  // a fused depth 0's miss radiance (PrimaryRays)
  for (int k = 0; k < 4; ++k) rp.missL[k] = 0.f;
  for (int j : G.hEnvLights) {
    const float* Le = G.hLights[j].L;
    for (int k = 0; k < 3; ++k) rp.missL[k] = rp.missL[k] + 1.0f * Le[k];
  }
  return rp;
}

// the request's sample table on g (GpuCtx::fcaches), built and uploaded at its first use
FrameCache& frame_cache(GpuCtx& g, const SampleRequest& req, uint64_t sceneSerial) {
  char keybuf[256];
  snprintf(keybuf, sizeof(keybuf), "%d/%d/%d/%d/%d/%s/%llu", req.spp, req.sets, req.iteration, req.num1D, req.num2D,
           req.filter.c_str(), (unsigned long long)sceneSerial);
  auto fit = g.fcaches.find(keybuf);
  if (fit == g.fcaches.end()) {
    if (g.fcaches.size() >= GpuCtx::kMaxFrameCaches) {
      g.fcaches.erase(g.fcacheOrder.front());
      g.fcacheOrder.pop_front();
    }
    auto fc = std::make_unique<FrameCache>();
    build_sample_table(req, fc->table);
    const SampleTable& t = fc->table;
    fc->slotLive.assign(t.numLightSlots, 0);
    for (int r = 0; r < t.numRecords; ++r)
      for (int k = 0; k < t.numLightSlots; ++k) {
        const float* ls = &t.light[((size_t)r * t.numLightSlots + k) * 8];
        if (!(ls[4] == 0.f && ls[5] == 0.f && ls[6] == 0.f)) fc->slotLive[k] = 1;
      }
    fc->dims.upload(fc->table.dims);
    fc->light.upload(fc->table.light);
    // the direction terms of the 2-D samples, computed on the device from the uploaded rows; the
    // lanes' streams read them, so the table is complete before the entry is used
    fc->dirs.alloc(sizeof(float4) * std::max<size_t>(1, (size_t)req.num2D * t.numRecords));
    launch_sample_dirs(fc->dims.as<float>() + (size_t)(5 + req.num1D) * t.numRecords, t.numRecords, req.num2D,
                       fc->dirs.as<float4>(), g.stream);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    fc->key = keybuf;
    g.fcacheOrder.push_back(keybuf);
    fit = g.fcaches.emplace(keybuf, std::move(fc)).first;
  }
  return *fit->second;
}

// direct lighting (pathtraceintegrator.cpp:123-167) skips a light whose sample radiance is
// exactly 0 for every sample of the frame (a zero L, e.g. C4's HDRILight L = 0 0 0): its
// shadow ray is never cast, so dropping it from the loop changes no pixel, and a frame left
// with one such light fuses the shadow resolve into the any-hit kernel. The loop keeps the
// lights' own indices (shadow jitter hash, light order).
static void direct_lights(GpuCtx& g, const GpuScene& G, const FrameCache& fcache, bool all, SceneView& sv) {
  g.hDirect.clear();
  for (int li = 0; li < (int)G.hLights.size(); ++li) {
    const GpuLight& lt = G.hLights[li];
    const bool live = lt.precomputed >= 0 ? (lt.precomputed < (int)fcache.slotLive.size() && fcache.slotLive[lt.precomputed])
                                          : !(lt.L[0] == 0.f && lt.L[1] == 0.f && lt.L[2] == 0.f);
    if (live || all) g.hDirect.push_back(li);
  }
  g.dDirect.alloc(sizeof(int) * std::max<size_t>(1, g.hDirect.size()));
  if (!g.hDirect.empty())
    HIP_CHECK(hipMemcpyAsync(g.dDirect.p, g.hDirect.data(), sizeof(int) * g.hDirect.size(), hipMemcpyHostToDevice,
                             g.stream));
  sv.directLights = g.dDirect.as<int>();
  sv.numDirectLights = (int)g.hDirect.size();
}

// Sizes g's frame block for nf W x H frames and, where the render's output is the shard
// (index, count) alone (`zero`), has the other shards' pixels read as zeros.
static void size_frame_block(GpuCtx& g, int W, int H, int nf, int index, int count, bool zero) {
  GpuCtx::FrameBlock& B = *g.blk;
  const void* const oldF = B.fbFloat.p;
  const void* const oldB = B.fbRGB8.p;
  const size_t floatBytes = B.float_bytes(W, H, nf), rgb8Bytes = B.rgb8_bytes(W, H, nf);
  B.fbFloat.alloc(floatBytes);
  B.fbRGB8.alloc(rgb8Bytes);
  const long long zkey[5] = {index, count, W, H, nf};
  if (B.fbFloat.p != oldF || B.fbRGB8.p != oldB) B.zeroKey[0] = -1;
  if (zero) {
    // pixels of other shards stay 0 so per-shard images compose by sum; a block that already
    // holds this layout's zeros (the same shard rendered into it before) is not cleared again.
    // Only ctx[0]'s block is output: the other devices of the process send their tiles to it.
    // Their (index, count) = (shardIndex, shardCount·N) identify the process's layout, since N
    // is fixed per Device (the debug renderer, which renders on ctx[0] alone, resets the key).
    if (memcmp(B.zeroKey, zkey, sizeof(zkey)) != 0) {
      HIP_CHECK(hipMemsetAsync(B.fbFloat.p, 0, floatBytes, g.stream));
      HIP_CHECK(hipMemsetAsync(B.fbRGB8.p, 0, rgb8Bytes, g.stream));
      memcpy(B.zeroKey, zkey, sizeof(zkey));
    }
  } else {
    B.zeroKey[0] = -1;  // every tile gets written (one shard, the gather, the debug renderer)
  }
}

// the frame as the kernels see it: the uploaded parameters, cameras, sample table and backplate
static FrameView frame_view(GpuCtx& g, const RendererObj& R, const FrameCache& fcache) {
  const SampleTable& tab = fcache.table;
  FrameView fv;
  fv.rp = g.dRp.as<GpuRenderParams>();
  fv.cam = g.dCam.as<GpuCamera>();
  fv.samples = fcache.dims.as<float>();
  fv.lightSamples = fcache.light.as<float>();
  fv.sampleDirs = fcache.dirs.as<float4>();
  fv.pixelSets = g.dPixelSets.as<uint8_t>();
  fv.numRecords = tab.numRecords;
  fv.numLightSlots = std::max(1, tab.numLightSlots);
  memset(&fv.backplate, 0, sizeof(fv.backplate));
  fv.backplateTexels = nullptr;
  if (R.backplate && !R.debug) {
    const ImageObj& im = *R.backplate;
    if (g.backplateSerial != im.serial) {
      g.dBackplate.upload(im.data);
      g.backplateSerial = im.serial;
    }
    fv.backplate.width = im.width;
    fv.backplate.height = im.height;
    fv.backplate.format = im.format;
    fv.backplate.offset = 0;
    fv.backplateTexels = g.dBackplate.as<uint8_t>();
  }
  return fv;
}

void Device::render_shard(GpuCtx& g, GpuScene& G, RendererObj& R, const std::vector<CameraObj*>& C,
                          ToneMapperObj& T, int W, int H, int index, int count, int accumulate, bool reportProgress,
                          float4* accu, const AdaptivePass* pass) {
  const int nf = (int)C.size();
  HIP_CHECK(hipSetDevice(g.hipDevice));
  memset(&g.stats, 0, sizeof(g.stats));
  g.accu = accu;
  if (!g.accu && !R.debug) {
    g.dJobAccu.alloc((size_t)nf * W * H * sizeof(float4));
    g.accu = g.dJobAccu.as<float4>();
  }
  ShardSetup s;
  s.sw = RenderSwitches::read();
  s.index = index;
  s.count = count;
  s.accumulate = accumulate;
  s.reportProgress = reportProgress;
  s.sv = G.view;
  s.sv.traceSpill = g.spill();
  const hipStream_t stream = g.stream;

  const SampleRequest req = sample_request(R, G);
  GpuRenderParams& rp = s.rp;
  rp = render_params(R, T, G, req, W, H, nf, frameSeed);
  const FrameCache& fcache = frame_cache(g, req, G.serial);
  rp.spp = fcache.table.spp;
  rp.sets = fcache.table.sets;
  direct_lights(g, G, fcache, s.sw.allDirectLights, s.sv);

  g.dRp.alloc(sizeof(rp));
  g.hCams.resize(nf);
  for (int k = 0; k < nf; ++k) g.hCams[k] = C[k]->cam;
  g.dCam.alloc(sizeof(GpuCamera) * nf);
  HIP_CHECK(hipMemcpyAsync(g.dRp.p, &rp, sizeof(rp), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemcpyAsync(g.dCam.p, g.hCams.data(), sizeof(GpuCamera) * nf, hipMemcpyHostToDevice, stream));
  g.dPixelSets.alloc((size_t)W * H);
  size_frame_block(g, W, H, nf, index, count, count > 1 && shardZero && &g == ctx[0].get() && !R.debug);
  s.fv = frame_view(g, R, fcache);

  if (reportProgress) status(R, 1, 0.f);
  const int numTiles = rp.tilesPerFrame * nf;
  s.shardTiles = pass ? pass->count : shard_tiles(numTiles, index, count);
  if (pass) {
    s.tileList = pass->tileList;
    s.half = pass->half;
  }

  if (R.debug) {
    launch_debug_render(s.sv, s.fv, R.maxDepth, R.spp, numTiles, g.fbFloat(), g.fbRGB8(), (int)rgb8_row_stride(W),
                        stream);
  } else {
    if (g.pixelSetsKey[0] != W || g.pixelSetsKey[1] != H || g.pixelSetsKey[2] != rp.sets) {
      launch_pixel_sets(s.fv, g.dPixelSets.as<uint8_t>(), W, H, rp.sets, stream);
      g.pixelSetsKey[0] = W;
      g.pixelSetsKey[1] = H;
      g.pixelSetsKey[2] = rp.sets;
    }
    const BatchPlan plan = plan_batches(s.shardTiles, rp.spp, capacity, g.numLanes, captureMax > 0, s.sw.batchGrow);
    ShardJob(*this, g, G, R, s, plan).run();
  }
  for (int l = 0; l < GpuCtx::kMaxLanes; ++l)
    if (g.lanes[l].stream) HIP_CHECK(hipStreamSynchronize(g.lanes[l].stream));
  g.stats.samples = (double)nf * W * H * (R.debug ? 1 : rp.spp);
}

}  // namespace yrt
