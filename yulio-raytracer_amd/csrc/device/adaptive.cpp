// adaptive.cpp — Device::render_adaptive (yrtRenderAdaptive): one frame in progressive
// iterations over the tiles that have not converged. Each iteration is a wavefront job over the
// active-tile list (Device::render_shard with an AdaptivePass); after every second one from
// minIterations on, k_tile_error estimates each active tile's error from the framebuffer's sums
// and half sums (common/yrt_tile_error.h) and k_tile_compact drops the tiles below the threshold
// from the list. The new count is the one value the host reads per check.
#include <chrono>
#include <cmath>
#include <limits>
#include <numeric>

#include "../common/yrt_tile_error.h"
#include "device.h"

namespace yrt {

float4* Device::frame_half(FrameBufferObj& F, GpuCtx& g) {
  for (const auto& a : F.adaptive)
    if (a->ctxSerial == g.serial) return a->half.as<float4>();
  HIP_CHECK(hipSetDevice(g.hipDevice));
  auto a = std::make_unique<FrameBufferObj::Adaptive>();
  a->ctxSerial = g.serial;
  a->half.alloc((size_t)F.width * F.height * sizeof(float4));
  F.adaptive.push_back(std::move(a));
  return F.adaptive.back()->half.as<float4>();
}

void Device::render_adaptive(RendererObj& R, CameraObj& C, SceneObj& S, ToneMapperObj& T, FrameBufferObj& F,
                             const YRTAdaptiveParams& p, YRTAdaptiveStats& out) {
  const auto t0 = std::chrono::steady_clock::now();
  // what the call cannot do is refused before anything is launched or changed
  if (p.maxIterations < 1) throw std::runtime_error("rtRenderAdaptive: maxIterations must be at least 1");
  if (!std::isfinite(p.threshold)) throw std::runtime_error("rtRenderAdaptive: the threshold is not finite");
  if (R.debug) throw std::runtime_error("rtRenderAdaptive: the debug renderer has no samples to adapt");
  if (shardCount > 1 || proc)
    throw std::runtime_error("rtRenderAdaptive: a tile shard, communicator or hub is armed (adaptive frames are "
                             "not gathered); drop it first");
  if (captureMax > 0) throw std::runtime_error("rtRenderAdaptive: ray capture is armed (yrtSetRayCapture)");
  if (ctx.size() > 1)
    throw std::runtime_error("rtRenderAdaptive: the device has " + std::to_string(ctx.size()) +
                             " render contexts (devices=...); adaptive frames render on one");
  if (!gpu) throw std::runtime_error("rtRenderAdaptive: host-only device (created with parms \"host\")");
  if (!S.gpu) throw std::runtime_error("scene not committed");
  if (S.gpu->device != hipDevice) throw std::runtime_error("scene committed on another HIP device");

  const int W = F.width, H = F.height;
  const int tilesX = (W + 15) / 16, tilesY = (H + 15) / 16, numTiles = tilesX * tilesY;
  const int minIterations = std::max(2, p.minIterations + (p.minIterations & 1));
  GpuCtx& g = *ctx[0];
  HIP_CHECK(hipSetDevice(g.hipDevice));
  memset(&stats, 0, sizeof(stats));
  R.iteration = 0;
  rotate_frame_block();
  GpuScene& G = scene_on(S, g.hipDevice, true);
  float4* const accu = frame_accu(F, g);
  float4* const half = frame_half(F, g);
  for (const auto& a : F.adaptive)
    if (a->ctxSerial == g.serial) {  // the display mapping of this render's resolves (render.cpp)
      a->gamma = T.gamma;
      a->rcpGamma = rcpf_(T.gamma);
      a->vignetting = T.vignetting;
    }
  HIP_CHECK(hipMemsetAsync(half, 0, (size_t)W * H * sizeof(float4), g.stream));

  // every tile active, in image order; no tile checked yet
  std::vector<int> list(numTiles);
  std::iota(list.begin(), list.end(), 0);
  F.tileIterations.assign(numTiles, 0);
  F.tileError.assign(numTiles, std::numeric_limits<float>::infinity());
  const size_t listBytes = (size_t)numTiles * sizeof(int);
  for (DevBuf& b : dTileList) b.alloc(listBytes);
  dTileStopped.alloc(listBytes);
  dTileIterations.alloc(listBytes);
  dTileError.alloc((size_t)numTiles * sizeof(float));
  dTileCount.alloc(sizeof(int));
  HIP_CHECK(hipMemcpyAsync(dTileList[0].p, list.data(), listBytes, hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipMemcpyAsync(dTileIterations.p, F.tileIterations.data(), listBytes, hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipMemcpyAsync(dTileError.p, F.tileError.data(), (size_t)numTiles * sizeof(float), hipMemcpyHostToDevice,
                           g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));  // the uploads read `list` and the framebuffer's vectors

  // the framebuffer holds neither a plain sequence nor, should an iteration throw, a whole frame
  F.accuFromAdaptive = true;
  F.accuFromJob = false;
  int active = numTiles, cur = 0, n = 0;
  double msError = 0, raysClosest = 0, raysShadow = 0, spp = R.spp;
  status(R, 1, 0.f);
  while (active > 0 && n < p.maxIterations && !(R.stopFlag && R.stopFlag->load())) {
    const int k = n;  // R.iteration
    const AdaptivePass pass{dTileList[cur].as<int>(), active, (k & 1) ? nullptr : half};
    render_shard(g, G, R, {&C}, T, W, H, 0, 1, k > 0, false, accu, &pass);
    spp = g.stats.samples / ((double)W * H);  // the sample table's
    raysClosest += g.stats.raysClosest;
    raysShadow += g.stats.raysShadow;
    R.iteration = n = k + 1;
    if (n % 2 == 0 && n >= minIterations) {
      const auto c0 = std::chrono::steady_clock::now();
      launch_tile_error(accu, half, W, H, tilesX, dTileList[cur].as<int>(), active, p.threshold, n,
                        dTileError.as<float>(), dTileIterations.as<int>(), dTileStopped.as<int>(), g.stream);
      launch_tile_compact(dTileList[cur].as<int>(), dTileStopped.as<int>(), active, dTileList[cur ^ 1].as<int>(),
                          dTileCount.as<int>(), g.stream);
      HIP_CHECK(hipGetLastError());
      int left = active;
      HIP_CHECK(hipMemcpyAsync(&left, dTileCount.p, sizeof(int), hipMemcpyDeviceToHost, g.stream));
      HIP_CHECK(hipStreamSynchronize(g.stream));
      if (left < 0 || left > active) throw std::runtime_error("rtRenderAdaptive: the compacted tile count is out of range");
      active = left;
      cur ^= 1;
      msError += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    }
    status(R, 1, float(n) / float(p.maxIterations));
  }

  // the tile records: a checked tile has its count from its last check; the tiles still active ran
  // every iteration
  HIP_CHECK(hipMemcpyAsync(F.tileIterations.data(), dTileIterations.p, listBytes, hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(F.tileError.data(), dTileError.p, (size_t)numTiles * sizeof(float), hipMemcpyDeviceToHost,
                           g.stream));
  if (active > 0)
    HIP_CHECK(hipMemcpyAsync(list.data(), dTileList[cur].p, (size_t)active * sizeof(int), hipMemcpyDeviceToHost,
                             g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  for (int j = 0; j < active; ++j) F.tileIterations[list[j]] = n;
  double samples = 0;
  for (int t = 0; t < numTiles; ++t)
    samples += (double)F.tileIterations[t] * spp * yrt_tile_pixels(t % tilesX, t / tilesX, W, H);

  hand_over_frames({&F}, W, H);
  stats.raysClosest = raysClosest;
  stats.raysShadow = raysShadow;
  stats.samples = samples;
  stats.msTotal = stats.msRender =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  out.iterations = n;
  out.tiles = numTiles;
  out.tilesStopped = numTiles - active;
  out.samples = samples;
  out.msTotal = stats.msTotal;
  out.msError = msError;
  status(R, 2, 1.f);
}

}  // namespace yrt
