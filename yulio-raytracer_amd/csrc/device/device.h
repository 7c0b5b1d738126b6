// device.h — the device plugin's host state, internal to csrc/device: the per-GPU state (GpuCtx),
// the Device class behind a YRTDevice handle and the guard macros of its C-ABI entry points.
//   device.cpp         Device's ray queries, frame read-back, scene commit
//   render.cpp         Device::render (the frame job), Device::render_shard (one device's share)
//   render_job.{h,cpp} the batch plan and the wavefront lane scheduler render_shard runs
//   adaptive.cpp       Device::render_adaptive (progressive iterations over the tiles not yet converged)
//   denoise.cpp        Device::guides, Device::denoise (a frame or a cube's faces), the cube-camera check
//   gather_device.cpp  Device::gather_local, Device::gather_process
//   api_objects.cpp, api_tools.cpp  the extern "C" entry points (include/yrt_device.h)
#pragma once

#include "../../../include/yrt_device.h"

#include <string.h>

#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../kernels/yrt_kernels.h"
#include "gather.h"
#include "objects.h"
#include "rccl_comm.h"
#include "sampler.h"
#include "scene_gpu.h"

namespace yrt {

// bytes of one row of an RGB8 frame: 3 bytes a pixel, rows padded to 4 bytes
inline size_t rgb8_row_stride(size_t width) { return (3 * width + 3) / 4 * 4; }

struct FrameCache {
  std::string key;
  SampleTable table;
  DevBuf dims, light;
  DevBuf dirs;  // the direction terms of the table's 2-D samples (k_sample_dirs), [num2D][numRecords] float4
  std::vector<uint8_t> slotLive;  // per light-sample slot: some record's radiance is not exactly 0
};

// One HIP device's rendering state: its streams (lanes), the frame buffers, the wavefront
// queues and the sample tables uploaded to it. A Device renders on one or several of these
// (yrtNewDevice "devices=..."): 16x16 tiles are dealt round-robin over them,
// one host thread drives each, and the frame is gathered on the first (rccl_comm.h).
struct GpuCtx {
  int hipDevice = 0;
  hipStream_t stream = nullptr;  // lanes[0].stream
  // A wavefront lane: a stream and the batch state it owns. Batches alternate between the
  // lanes so one batch's kernels run beside the other's (the VALU-bound traversal next to the
  // latency-bound shading).
  struct Lane {
    hipStream_t stream = nullptr;
    DevBuf qPath[2], qOrg[2], qDir[2], qThr[2], hit, pathL, shFirst, sOrg, sDir, sContrib, sOcc, counters, spill;
    DevBuf qTime[2], sTime;  // ray times (moving scenes only)
    int64_t pathCap = 0, shadowCap = 0;
    // Batches enqueued whose queue counters are not yet accounted, oldest first: a pinned
    // copy of the counters (written by the stream after the batch's last trace), the event
    // after that copy, the batch's tiles (progress) and its place in the job (seq). A lane
    // takes its next batch once its previous batch's counters have arrived — before that
    // batch's pixel resolve, so the host enqueues while the resolve runs. Two batches ahead
    // per lane measured the same (profiles/r04/ab_r04k.txt).
    struct Pend {
      unsigned* hc = nullptr;
      size_t hcWords = 0;
      hipEvent_t done = nullptr;
      int64_t tiles = 0;
      int64_t seq = 0;
      bool fused = false;  // depth 0 ran as k_trace's camera-ray instantiation (hits queued only)
    };
    static constexpr int kPendDepth = 1;
    Pend pend[kPendDepth];
    int pendHead = 0, pendCount = 0;
  };
#ifndef YRT_MAX_LANES
#define YRT_MAX_LANES 4  // one HIP stream each; HIP gives a process 4 hardware queues by default
#endif
  static constexpr int kMaxLanes = YRT_MAX_LANES;  // YRT_LANES may ask for up to this many
  // three: a process gets 4 hardware queues (GPU_MAX_HW_QUEUES), and four lane streams plus the
  // context's own stream (clears, copies, the gather) share them. Same box against four
  // (profiles/r06/ab_r06r.txt): C3 +3.4 %, C4 cube job -1.7 %, C5 -2.7 %, N = 8 rank shares C3
  // -13.5 % (slowest) and C4 -5 %. (Round 5: four over two C3 +1.4 %, ab_lanes_r05q.txt; rounds
  // 1-2: two +4 % over one.)
  static constexpr int kDefaultLanes = 3;
  static int default_lanes() {
    int lanes = kDefaultLanes;
    if (const char* e = getenv("YRT_LANES")) lanes = std::max(1, std::min(kMaxLanes, atoi(e)));
    return lanes;
  }
  Lane lanes[kMaxLanes];
  int numLanes = kDefaultLanes;
  DevBuf dRp, dCam, dPixelSets, dCount, dSpill, dSlab, dDirect;
  // The (sum, weight) pixels the job's pixel resolve reads and writes (k_resolve_pixels): the
  // framebuffer's own sums on this context (FrameBufferObj::accu) for a one-frame job; a
  // multi-frame job never accumulates, so its frames' sums go to the scratch block dJobAccu
  float4* accu = nullptr;
  DevBuf dJobAccu;
  // names this context in FrameBufferObj::Accu (an address could be a later context's)
  const uint64_t serial = next_serial();
  static uint64_t next_serial() {
    static std::atomic<uint64_t> n{0};
    return ++n;
  }
  // denoise (yrtRenderGuides / yrtDenoiseFrameBuffer / yrtDenoiseCube), per face of the surface:
  // the guide frames, the filter's two ping-pong float4 frames, the modulation, the uploads of the
  // frames that live in host pixels and the FrameIO records; the cameras go to dCam
  DevBuf dGuidePos, dGuideNrm, dGuideAlbedo, dFilter[2], dFilterMod, dFilterFb, dFaceIo;
  // the variance frames (var4) of the variance-guided filter and of yrtFrameVariance
  DevBuf dFilterVar;
  // The frames a job renders into (float RGB and RGB8 rows, frame-major). On the primary
  // device a job's framebuffers keep a reference to their block until rtMapFrameBuffer reads
  // them back, so the next job renders into the spare (or a fresh) block meanwhile.
  struct FrameBlock {
    DevBuf fbFloat, fbRGB8;
    // the shard layout (index, count, width, height, frames) whose other shards' pixels this
    // block holds as zeros (a one-shard render writes only its own tiles); -1: unknown
    long long zeroKey[5] = {-1, -1, -1, -1, -1};
    // bytes of `frames` W x H frames in fbFloat / fbRGB8 (frame k starts at k times one frame's)
    static size_t float_bytes(int W, int H, int frames) { return (size_t)frames * W * H * 3 * sizeof(float); }
    static size_t rgb8_bytes(int W, int H, int frames) { return (size_t)frames * rgb8_row_stride(W) * H; }
  };
  std::shared_ptr<FrameBlock> blk = std::make_shared<FrameBlock>(), spareBlk;
  // every block allocated after the first two (weak: a block lives while a framebuffer's
  // unread frame or blk / spareBlk holds it); at most kMaxFrameBlocks stay alive
  static constexpr int kMaxFrameBlocks = 3;
  std::vector<std::weak_ptr<FrameBlock>> extraBlocks;
  float* fbFloat() const { return blk->fbFloat.as<float>(); }
  uint8_t* fbRGB8() const { return blk->fbRGB8.as<uint8_t>(); }
  std::vector<int> hDirect;        // the frame's direct-light list (uploaded to dDirect)
  std::vector<GpuCamera> hCams;  // the job's cameras, one per frame (uploaded to dCam)
  DevBuf dBackplate;                       // the renderer's backplate image (texels)
  uint64_t backplateSerial = 0;            // ImageObj::serial of the image dBackplate holds
  // (width, height, sets) of the pixel-set map dPixelSets holds: the map depends on nothing else
  // (integratorrenderer.cpp:126-131 seeds by tile position), so a frame of the same size reuses it
  long long pixelSetsKey[3] = {-1, -1, -1};
  // per committed scene (GpuScene::serial): camera rays traced by fused depth-0 batches
  // (launch_trace_primary) and how many of them left the scene; their ratio picks the depth-0
  // kernels (a running total: one batch's share varies with the faces it covers)
  std::map<uint64_t, std::pair<double, double>> missFrac;
  std::map<int, DevBuf> recvSlabs;  // gather on the first device: one slab per peer
  // sample tables by request (a progressive or multi-GPU weak-scaling run cycles through a
  // few sampler iterations; rebuilding a table costs ~9 ms of host time per frame)
  static constexpr size_t kMaxFrameCaches = 16;
  std::map<std::string, std::unique_ptr<FrameCache>> fcaches;
  std::deque<std::string> fcacheOrder;
  std::vector<hipEvent_t> eventPool;
  YRTRenderStats stats{};
  struct Captured { std::vector<float> org, dir; double total = 0; };
  std::vector<Captured> capClosest, capShadow;

  GpuCtx(int dev, int lanesWanted) : hipDevice(dev), numLanes(lanesWanted) {
    HIP_CHECK(hipSetDevice(hipDevice));
    ensure_streams(1);
    stream = lanes[0].stream;
  }
  // A lane's stream is created when a render first uses the lane: several contexts
  // in one process (e.g. devices=[0,0]) all map their lanes onto the process's 4 hardware queues
  // (GPU_MAX_HW_QUEUES), so streams nobody renders on only add to that sharing.
  void ensure_streams(int n) {
    for (int l = 0; l < n && l < kMaxLanes; ++l)
      if (!lanes[l].stream) HIP_CHECK(hipStreamCreateWithFlags(&lanes[l].stream, hipStreamNonBlocking));
  }
  ~GpuCtx() {
    (void)hipSetDevice(hipDevice);
    for (auto e : eventPool) (void)hipEventDestroy(e);
    for (Lane& L : lanes) {
      for (Lane::Pend& P : L.pend) {
        if (P.hc) (void)hipHostFree(P.hc);
        if (P.done) (void)hipEventDestroy(P.done);
      }
      if (L.stream) (void)hipStreamDestroy(L.stream);
    }
  }
  hipEvent_t ev() {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    eventPool.push_back(e);
    return e;
  }
  int* spill() {
    dSpill.alloc(YRT_TRACE_SPILL_INTS * sizeof(int));
    return dSpill.as<int>();
  }
  // P paths per batch; queues hold YRT_QSEGS segments of qseg_capacity(P) slots
  static void ensure_paths(Lane& L, int64_t P, int numLights, bool motion) {
    const int64_t Q = (int64_t)YRT_QSEGS * qseg_capacity(P);
    if (Q > L.pathCap) {
      for (int k = 0; k < 2; ++k) {
        L.qPath[k].alloc(Q * 4);
        L.qOrg[k].alloc(Q * 16);
        L.qDir[k].alloc(Q * 16);
        L.qThr[k].alloc(Q * 16);
      }
      L.hit.alloc(Q * 16);
      L.pathL.alloc(Q * 16);
      L.pathCap = Q;
    }
    const int64_t S = Q * std::max(1, numLights);
    if (S > L.shadowCap) {
      L.shFirst.alloc(S * 4);
      L.sOrg.alloc(S * 16);
      L.sDir.alloc(S * 16);
      L.sContrib.alloc(S * 16);
      L.sOcc.alloc(S * 4);
      L.shadowCap = S;
    }
    if (motion) {
      for (int k = 0; k < 2; ++k) L.qTime[k].alloc(Q * 4);
      L.sTime.alloc(S * 4);
    }
  }
  // ray capture (roofline accounting): strided sample of each depth's query streams, batch 0
  // counts: the queue's first segment counter; segments of segCap slots
  void capture(int captureMax, std::vector<Captured>& out, int depth, const float4* org, const float4* dir,
               const unsigned* counts, int segCap, hipStream_t st) {
    std::vector<unsigned> cs((size_t)YRT_QSEGS * YRT_QCSTRIDE);
    HIP_CHECK(hipMemcpyAsync(cs.data(), counts, cs.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    size_t n = 0;
    for (int k = 0; k < YRT_QSEGS; ++k) n += cs[(size_t)k * YRT_QCSTRIDE];
    if ((int)out.size() <= depth) out.resize(depth + 1);
    Captured& c = out[depth];
    c.total = (double)n;
    c.org.clear();
    c.dir.clear();
    const size_t stride = std::max<size_t>(1, (n + captureMax - 1) / captureMax);
    for (int k = 0; k < YRT_QSEGS; ++k) {
      const size_t nk = cs[(size_t)k * YRT_QCSTRIDE];
      const size_t m = nk ? (nk + stride - 1) / stride : 0;
      if (!m) continue;
      const size_t at = c.org.size();
      c.org.resize(at + m * 4);
      c.dir.resize(at + m * 4);
      HIP_CHECK(hipMemcpy2D(c.org.data() + at, 16, org + (size_t)k * segCap, stride * 16, 16, m,
                            hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy2D(c.dir.data() + at, 16, dir + (size_t)k * segCap, stride * 16, 16, m,
                            hipMemcpyDeviceToHost));
    }
  }
};

// the request's sample table on g (GpuCtx::fcaches), built and uploaded at its first use (render.cpp)
FrameCache& frame_cache(GpuCtx& g, const SampleRequest& req, uint64_t sceneSerial);

// the tiles of shard (index, count): tile = index + j * count, j < shard_tiles
inline int shard_tiles(int numTiles, int index, int count) {
  return numTiles > index ? (numTiles - index + count - 1) / count : 0;
}

// Copies the frame framebuffer F's buffer `id` still holds in HBM (FrameBufferObj::Pending)
// into its host pixels, converting float RGB to the RGBA / RGBA8 formats.
void fb_read_back(FrameBufferObj& F, int id);

inline void status(RendererObj& R, int state, float progress) {
  if (R.statusCallback) ((YRTStatusCallback)R.statusCallback)(state, progress, R.statusUser);
}

// yrtSetKernelTiming: the HIP-event time of what `time` enqueues on a stream (one launch of a
// render step; the guide pass; the filter's load and iterations). With timing off no event is
// created or recorded. The events are read once the stream has been synchronized.
struct EvPair {
  hipEvent_t a = nullptr, b = nullptr;
  EvPair() = default;
  EvPair(EvPair&& o) noexcept : a(o.a), b(o.b) { o.a = o.b = nullptr; }
  EvPair(const EvPair&) = delete;
  EvPair& operator=(const EvPair&) = delete;
  ~EvPair() { reset(); }
  void reset() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
  }
  template <class Launch>
  void time(bool on, hipStream_t st, Launch&& launch) {
    reset();  // a call that threw before its read
    if (on) {
      HIP_CHECK(hipEventCreate(&a));
      HIP_CHECK(hipEventCreate(&b));
      HIP_CHECK(hipEventRecord(a, st));
    }
    launch();
    if (b) HIP_CHECK(hipEventRecord(b, st));
  }
  // after the stream's synchronize; leaves ms as it is when timing is off
  void read(float& ms) {
    if (b) HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    reset();
  }
};

class Device {
 public:
  std::recursive_mutex mu;
  std::string lastError;
  std::set<HandleRef*> handles;
  std::vector<std::unique_ptr<GpuCtx>> ctx;  // ctx[0]: the primary device (commits, queries, output)
  int hipDevice = 0;                         // ctx[0]'s
  hipStream_t stream = nullptr;              // ctx[0]'s
  uint32_t frameSeed = 0x2545F491u;
#ifndef YRT_DEFAULT_CAPACITY_M
#define YRT_DEFAULT_CAPACITY_M 64
#endif
  int64_t capacity = (int64_t)YRT_DEFAULT_CAPACITY_M << 20;  // paths per batch: C3 +4 % over 16 M (fewer launch tails), ~10 GB
  // process-level shard (yrtSetTileShard / yrtSetShardComm): this process renders tiles
  // t = shardIndex (mod shardCount), dealt over its own devices
  int shardIndex = 0, shardCount = 1;
  // process-level gather to rank 0 (gather.h): RCCL (yrtSetShardComm) or an in-process hub
  // of several Device objects (yrtSetShardHub)
  std::unique_ptr<GatherTransport> proc;
  int commRank = 0, commWorld = 1;   // proc's rank / size: the only shard it gathers
  double gatherTimeout = default_gather_timeout();  // bound of every gather wait (yrtSetGatherTimeout)
  ncclComm_t localComm = nullptr;    // the ctx devices' gather (distinct devices only): rank 0's
  std::vector<ncclComm_t> localComms;  // one per ctx device (ncclCommInitAll)
  // ncclCommInitAll failed (or a gather over it timed out): distinct devices gather with
  // hipMemcpyPeerAsync instead, reported as YRT_GATHER_PEER_COPY in the render stats
  bool localRcclOff = getenv("YRT_NO_LOCAL_RCCL") != nullptr;
  std::string localRcclWhy;
  bool refitCommits = true;  // SceneObj::commit refits faceCamera-only changes (yrtSetRefitCommits)
  bool kernelTiming = false;
  YRTRenderStats stats{};
  int captureMax = 0;

  bool gpu = true;  // false: host-only device (loaders, BVH, export; no rendering) for CPU tests
  Device(const std::vector<int>& devs, bool useGpu);
  DevBuf dbgPixelBuf;   // yrtDebugPixelSamples capture (a debugging aid), armed on this device
  int dbgPixelCap = 0;
  ~Device();

  YRTHandle wrap(std::shared_ptr<Object> o);
  HandleRef* ref(YRTHandle h);
  template <class T>
  std::shared_ptr<T> get(YRTHandle h, const char* what) {
    if (!h) return nullptr;
    auto o = std::dynamic_pointer_cast<T>(ref(h)->obj);
    if (!o) throw std::runtime_error(std::string("invalid ") + what + " handle");
    return o;
  }

  int* spill() { return ctx[0]->spill(); }

  // the committed scene as seen by one of the devices (a peer copy, refreshed after rebuilds
  // and refits; logical shards on the primary's own device share its buffers)
  // YRT_FORCE_SCENE_REPLICA=1 (tests): peer-copy the scene even onto the primary's own device,
  // so a one-GPU box exercises the replication path of multi-GPU renders
  GpuScene& scene_on(SceneObj& S, int dev, bool primary);

  // one or several frames of the same size and format in one wavefront job (yrtRenderFrames):
  // their tiles form one sequence, frame-major, dealt over shards and devices
  void render(RendererObj& R, const std::vector<CameraObj*>& C, SceneObj& S, ToneMapperObj& T,
              const std::vector<FrameBufferObj*>& F, int accumulate);
  // makes ctx[0]->blk a frame block no framebuffer holds unread frames in
  void rotate_frame_block();
  // the W x H frames a job rendered into ctx[0]->blk, frame k to F[k]: each framebuffer keeps a
  // reference to its frame in HBM (FrameBufferObj::Pending) or, with user pixels, reads it back now
  void hand_over_frames(const std::vector<FrameBufferObj*>& F, int W, int H);
  // F's accumulation buffer on g, created cleared (enqueued on g's stream) at g's first frame
  // into F; later frames only look it up
  static float4* frame_accu(FrameBufferObj& F, GpuCtx& g);
  // Renders the tiles of shard (index, count) of the frame into g's full-size buffers (the other
  // tiles' pixels are left zero when count > 1). accu: the framebuffer's accumulation buffer on g
  // (frame_accu) of a one-frame job, null for a multi-frame job or the debug renderer.
  // pass: one iteration of an adaptive render, the listed tiles of the whole frame (index 0, count 1).
  struct AdaptivePass {
    const int* tileList;  // device array: the active image tiles, ascending
    int count;
    float4* half;         // the half buffer this iteration is also added into, or null
  };
  void render_shard(GpuCtx& g, GpuScene& G, RendererObj& R, const std::vector<CameraObj*>& C, ToneMapperObj& T,
                    int W, int H, int index, int count, int accumulate, bool reportProgress, float4* accu,
                    const AdaptivePass* pass = nullptr);
  // yrtRenderAdaptive (adaptive.cpp): one frame in progressive iterations of R.spp samples, each
  // over the tiles whose error estimate (common/yrt_tile_error.h) has not fallen below p.threshold
  void render_adaptive(RendererObj& R, CameraObj& C, SceneObj& S, ToneMapperObj& T, FrameBufferObj& F,
                       const YRTAdaptiveParams& p, YRTAdaptiveStats& out);
  // F's half buffer on g (FrameBufferObj::Adaptive), allocated at g's first adaptive render into F
  static float4* frame_half(FrameBufferObj& F, GpuCtx& g);
  // device scratch of the adaptive check: two tile lists, stop flags, the records, the count word
  DevBuf dTileList[2], dTileStopped, dTileError, dTileIterations, dTileCount;
  int gather_local(const SlabLayout& base, int numTiles);
  // the render's output is this shard alone (no gather fills the other shards' tiles): those
  // pixels must read as zeros, so per-shard images compose by sum
  bool shardZero = true;
  // renderSeconds: this rank's render time of the call; the status exchange waits for the
  // slowest rank's render, so its deadline is gatherTimeout + kStatusRenderFactor x that time
  // (a peer may take ten times as long before the gather gives up; the slab transfers keep
  // gatherTimeout)
  static constexpr double kStatusRenderFactor = 10.0;
  void gather_process(const SlabLayout& base, int numTiles, bool localOk, double renderSeconds);
  // copies every unread frame held in block b into its framebuffer's host pixels
  void read_back_block(const void* b);
  // a process gather is armed: every render of this device joins the ranks' status exchange
  bool proc_gather_armed() const {
    return proc && shardCount > 1 && shardIndex == commRank && shardCount == commWorld;
  }
  // A render call that fails before reaching render() (bad handles, host-only device) still
  // joins the status exchange with flag 0, so the peers fail instead of waiting for it.
  void fail_proc_gather();
  // yrtIntersect / yrtOccluded (occ set: any hit); time: one float per ray or null (the untimed
  // call), ignored by a scene without moving geometry
  void intersect(SceneObj& S, const float* org4, const float* dir4, const float* time, uint32_t n, float* hit4,
                 int32_t* occ, hipStream_t st);
  // the first-hit guide frames of the W x H views of C (one frame: one camera) as [face][H][W]
  // arrays in ctx[0]'s dGuidePos / dGuideNrm (enqueued on the primary stream); albedo: the same
  // pass also fills dGuideAlbedo (k_guides<true>). Checks the scene and the pixel count.
  void guides(const std::vector<CameraObj*>& C, SceneObj& S, int W, int H, const char* what, bool albedo);
  // yrtSetKernelTiming: HIP-event times of the last guide pass and the last filter (its load and
  // iterations), yrtGetDenoiseTimes
  EvPair evGuides, evFilter;
  float msGuides = 0.f, msFilter = 0.f;
  // the filter over the frames F[k] of one size and format seen through C[k], in place: one frame,
  // or (wrap) the validated slots k = eye * 6 + face of a stereo cube filtered as one surface
  void denoise(const std::vector<CameraObj*>& C, SceneObj& S, const std::vector<FrameBufferObj*>& F,
               const YRTDenoiseParams& p, bool wrap, const char* what);
  // where buffer `id` of F lives for the filter: in this device's frame block, or on the host
  struct FilterFrame {
    FrameIO io;
    bool inBlock;
  };
  FilterFrame filter_frame(FrameBufferObj& F, int id);
  // what k_frame_variance reads of F on ctx[0]: the sums and half sums of its last adaptive render
  // and that render's display mapping; throws (naming `what`) unless F's last frame is an adaptive
  // render on ctx[0] whose tiles all ran two iterations or more
  struct VarianceSource {
    const float4* accu = nullptr;
    const float4* half = nullptr;
    float gamma = 1.f, rcpGamma = 1.f;
    int vignetting = 0;
  };
  VarianceSource variance_source(FrameBufferObj& F, const char* what);
  // yrtFrameVariance: var4 ([H][W][4] floats) of F's last adaptive render to the host
  void frame_variance(FrameBufferObj& F, float* var4Host);
};

// yrtDenoiseCube's host check: empty when the six faces of a committed stereo camera are the ideal
// cube's (denoise.cpp), otherwise what is wrong
std::string cube_cameras_defect(const GpuCamera& cam);

}  // namespace yrt

// ---------------------------------------------------------------- C ABI
struct YRTDevice_ {
  yrt::Device* d;
};

#define DEV_GUARD(dev, failret)                                         \
  if (!dev || !dev->d) return failret;                                  \
  std::lock_guard<std::recursive_mutex> _lk(dev->d->mu);                \
  try {
#define DEV_END(failret)                                                \
  }                                                                     \
  catch (const std::exception& e) {                                     \
    dev->d->lastError = e.what();                                       \
    return failret;                                                     \
  }
