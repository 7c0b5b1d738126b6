// render_job.h — the wavefront job Device::render_shard runs on one GPU: how the shard's tiles
// are cut into batches (plan_batches) and the scheduler that enqueues the batches' kernels over
// the GPU's lanes (ShardJob).
#pragma once

#include "device.h"

namespace yrt {

// The render-time environment switches, read once per render_shard call (never kept across
// calls: a process may change them between two renders).
struct RenderSwitches {
  int primary;            // YRT_PRIMARY: fused depth 0 never (0), by the measured miss share (1), always (2)
  double primaryMiss;     // YRT_PRIMARY_MISS: the miss share from which a batch's depth 0 is fused
  bool noShadowFuse;      // YRT_NO_SHADOW_FUSE: one direct light still gets its shadow resolve pass
  bool allDirectLights;   // YRT_ALL_DIRECT_LIGHTS: zero-radiance lights stay in the direct-light list
  bool batchGrow;         // YRT_BATCH_GROW=0: off
  static RenderSwitches read();
};

struct BatchPlan {
  int64_t tilesPerBatch, numBatches, pathsPerBatch;
  int lanes;  // lanes the job runs on
};
// capture: the capture frame (yrtSetRayCapture); grow: RenderSwitches::batchGrow
BatchPlan plan_batches(int64_t shardTiles, int spp, int64_t capacity, int numLanes, bool capture, bool grow);

// What render_shard has set up for the job: the scene and frame as the kernels see them, and
// the shard (index, count) of shardTiles tiles.
struct ShardSetup {
  SceneView sv;
  FrameView fv;
  GpuRenderParams rp;
  RenderSwitches sw;
  int index, count, shardTiles, accumulate;
  bool reportProgress;
  // An adaptive render's iteration (adaptive.cpp): the shard is the shardTiles image tiles of
  // tileList (a device array, ascending) instead of an arithmetic sequence, and every batch is
  // also added into the half buffer when that is not null. null: a plain job.
  const int* tileList = nullptr;
  float4* half = nullptr;
};

class ShardJob {
 public:
  ShardJob(const Device& D, GpuCtx& g, const GpuScene& G, RendererObj& R, const ShardSetup& s, const BatchPlan& plan);
  // enqueues every batch of the shard and accounts their queue counters; the lanes' last pixel
  // resolves may still run when it returns
  void run();

 private:
  using Lane = GpuCtx::Lane;
  // a lane's view of the job (built once, prepare_lanes) and the batch it is enqueueing
  struct LaneJob {
    PathBuffers pb;
    SceneView sv;  // s.sv with the lane's own trace spill buffer
    bool active = false;
    int step = 0;  // 0: prologue, 1..maxDepth: depth step - 1, maxDepth + 1: epilogue
    int64_t first = 0, seq = 0;
    BatchInfo bi{};
    bool fused = false;
  };
  void prepare_lanes();
  PathBuffers lane_buffers(Lane& L) const;
  bool drain_one(Lane& L, bool wait);
  void start_batches();
  void enqueue_step(Lane& L, LaneJob& J);
  template <class Launch>
  void timed(double YRTRenderStats::*sum, hipStream_t st, Launch&& launch);

  GpuCtx& g;
  const GpuScene& G;
  RendererObj& R;
  const ShardSetup& s;
  const BatchPlan plan;
  const bool kernelTiming;
  const int captureMax;
  const int levels;           // queue levels: maxDepth + 1
  // the queue counters, then one word: the camera rays a fused depth 0 traced
  // (PrimaryRays::traced)
  const size_t counterWords, tracedWord;
  const int numDirect;
  bool fusedPrimary = false;  // the job's batches may run depth 0 fused (see run())
  double missEst = -1.0;      // the scene's measured camera-ray miss share (GpuCtx::missFrac); < 0: unknown
  int64_t tilesDone = 0, batch = 0;
  int64_t nextFirst = 0;  // the next batch's first tile of the shard
  std::vector<LaneJob> jobs;  // one per lane
  struct Timed { EvPair ev; double YRTRenderStats::*sum; };
  std::vector<Timed> evs;
};

}  // namespace yrt
