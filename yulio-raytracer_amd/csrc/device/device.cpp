// device.cpp — the MI355X device plugin's Device: construction, handle bookkeeping, the scene
// as seen by each of its GPUs, frame read-back, ray queries and the scene commit. The frame
// renderer, the denoise stage, the gathers and the C-ABI entry points are in the files device.h
// lists.
//
// Reference counterparts: SingleRayDevice (device_singleray/api/singleray_device.cpp:99-709),
// IntegratorRenderer::renderFrame/RenderJob (renderers/integratorrenderer.cpp:63-185),
// DebugRenderer (renderers/debugrenderer.cpp:66-140).
#include "device.h"

namespace yrt {

#ifndef YRT_STACK_DEPTH
#define YRT_STACK_DEPTH 64
#endif

Device::Device(const std::vector<int>& devs, bool useGpu) : gpu(useGpu) {
  if (!gpu) return;
  const int lanes = GpuCtx::default_lanes();
  for (int d : devs) ctx.emplace_back(new GpuCtx(d, lanes));
  hipDevice = ctx[0]->hipDevice;
  stream = ctx[0]->stream;
  HIP_CHECK(hipSetDevice(hipDevice));
}

Device::~Device() {
  if (dbgPixelBuf.p) (void)debug_pixel_capture(-1, -1, nullptr, 0);  // no kernel may write it once freed
  for (auto* h : handles) delete h;
  handles.clear();
  try {
    for (auto c : localComms) rccl().CommDestroy(c);
  } catch (...) {
  }
  proc.reset();
}

YRTHandle Device::wrap(std::shared_ptr<Object> o) {
  o->dev = this;
  auto* h = new HandleRef();
  h->obj = std::move(o);
  handles.insert(h);
  return (YRTHandle)h;
}

HandleRef* Device::ref(YRTHandle h) {
  auto* r = (HandleRef*)h;
  if (!r || handles.find(r) == handles.end()) throw std::runtime_error("invalid handle");
  return r;
}

GpuScene& Device::scene_on(SceneObj& S, int dev, bool primary) {
  // read per call: a process that has rendered before (a test suite) can still switch it on
  const bool force = getenv("YRT_FORCE_SCENE_REPLICA") != nullptr;
  if (dev == S.gpu->device && (primary || !force)) return *S.gpu;
  auto& r = S.replicas[dev];
  if (!r || r->serial != S.gpu->serial || r->refits != S.gpu->refits) r = replicate_gpu_scene(*S.gpu, dev);
  return *r;
}

void Device::read_back_block(const void* b) {
  for (HandleRef* h : handles)
    if (auto* F = dynamic_cast<FrameBufferObj*>(h->obj.get()))
      for (int id = 0; id < (int)F->pending.size(); ++id)
        if (F->pending[id].keep.get() == b) fb_read_back(*F, id);
}

void Device::fail_proc_gather() {
  if (!proc_gather_armed() || proc->aborted()) return;
  try {
    (void)proc->exchange_status(0, hipDevice, stream, gatherTimeout);
  } catch (...) {
  }
}

void fb_read_back(FrameBufferObj& F, int id) {
  if (id < 0 || id >= (int)F.pending.size() || !F.pending[id].keep) return;
  FrameBufferObj::Pending pf = F.pending[id];
  F.pending[id] = FrameBufferObj::Pending();
  HIP_CHECK(hipSetDevice(pf.hipDevice));
  const int W = F.width, H = F.height;
  void* dst = F.buffer(id);
  if (F.format == FB_RGB8) {
    HIP_CHECK(hipMemcpy(dst, pf.src, F.stride * H, hipMemcpyDeviceToHost));
    return;
  }
  if (F.format == FB_RGB_FLOAT32) {
    HIP_CHECK(hipMemcpy(dst, pf.src, (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return;
  }
  std::vector<float> tmp((size_t)W * H * 3);
  HIP_CHECK(hipMemcpy(tmp.data(), pf.src, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
  if (F.format == FB_RGBA_FLOAT32) {
    float* o = (float*)dst;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
      o[4 * i] = tmp[3 * i]; o[4 * i + 1] = tmp[3 * i + 1]; o[4 * i + 2] = tmp[3 * i + 2]; o[4 * i + 3] = 1.0f;
    }
  } else {  // RGBA8: pixel[3] = 0 (framebuffer.h:170-178)
    uint8_t* o = (uint8_t*)dst;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
      for (int c = 0; c < 3; ++c) o[4 * i + c] = (uint8_t)clampf(tmp[3 * i + c] * 255.0f, 0.0f, 255.0f);
      o[4 * i + 3] = 0;
    }
  }
}

// ---------------------------------------------------------------- ray queries
void Device::intersect(SceneObj& S, const float* org4, const float* dir4, const float* time, uint32_t n, float* hit4,
                       int32_t* occ, hipStream_t st) {
  if (!gpu) throw std::runtime_error("ray query: host-only device (created with parms \"host\")");
  HIP_CHECK(hipSetDevice(hipDevice));
  if (!S.gpu) throw std::runtime_error("scene not committed");
  // a static scene has no triMotion records and ignores the rays' times (Ray::time is not read by
  // a static mesh): the static kernels run, and `time` is never dereferenced
  if (!S.gpu->hasMotion) time = nullptr;
  GpuCtx& g = *ctx[0];
  g.dCount.alloc(sizeof(unsigned));
  HIP_CHECK(hipMemcpyAsync(g.dCount.p, &n, sizeof(unsigned), hipMemcpyHostToDevice, st));
  SceneView sv = S.gpu->view;
  sv.traceSpill = spill();
  if (occ)
    launch_trace_any(sv, (const float4*)org4, (const float4*)dir4, g.dCount.as<unsigned>(), 1, (int)n, occ, st, nullptr,
                     time);
  else
    launch_trace_closest(sv, (const float4*)org4, (const float4*)dir4, g.dCount.as<unsigned>(), 1, (int)n,
                         (float4*)hit4, st, time);
  HIP_CHECK(hipStreamSynchronize(st));
}

// ---------------------------------------------------------------- scene commit
void SceneObj::commit() {
  std::vector<std::shared_ptr<ScenePrim>> prims = slots;
  Device* d = static_cast<Device*>(dev);
  // scene property "builder" (api/scene.h:45): "morton" builds the BVH on the GPU (bvh_build.h),
  // every other value is the host SAH builder; YRT_BUILDER=morton makes "default" mean "morton"
  const Variant* bv = parms.find("builder");
  std::string builder = bv && bv->type == Variant::STRING ? bv->str : "default";
  if (builder == "default") {
    const char* env = getenv("YRT_BUILDER");
    if (env) builder = env;
  }
  const bool morton = builder == "morton";
  // per-face commits of the FPR loop (renderer.cpp:550-559) only re-orient faceCamera
  // meshes: refit on the GPU instead of rebuilding; a tree of the other
  // builder is never refit
  if (gpu && d->gpu && d->refitCommits && gpu->mortonAsked == morton) {
    HIP_CHECK(hipSetDevice(d->hipDevice));
    if (refit_gpu_scene(*gpu, prims, d->stream)) return;
  }
  if (morton && d->gpu) HIP_CHECK(hipSetDevice(d->hipDevice));  // the build's kernels run in d->stream
  gpu = build_gpu_scene(prims, YRT_STACK_DEPTH, d->gpu, morton, d->gpu ? d->stream : nullptr, d->kernelTiming);
}

}  // namespace yrt
