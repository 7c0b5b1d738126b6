// denoise.cpp — the denoise stage of the device plugin: the first-hit guide pass (yrtRenderGuides,
// yrtRenderAlbedo) and the edge-avoiding a-trous filter over a rendered frame
// (yrtDenoiseFrameBuffer).
#include "device.h"

namespace yrt {

void Device::guides(CameraObj& C, SceneObj& S, int W, int H, const char* what, bool albedo) {
  if (!S.gpu) throw std::runtime_error(std::string(what) + ": scene not committed");
  if (S.gpu->device != hipDevice) throw std::runtime_error(std::string(what) + ": scene committed on another HIP device");
  // one thread per pixel in 64-lane blocks: the grid stays far inside 2^31 blocks
  if ((long long)W * H > (1ll << 30)) throw std::runtime_error(std::string(what) + ": more than 2^30 pixels");
  HIP_CHECK(hipSetDevice(hipDevice));
  GpuCtx& g = *ctx[0];
  const size_t bytes = (size_t)W * H * sizeof(float4);
  g.dCam.alloc(sizeof(GpuCamera));
  g.dGuidePos.alloc(bytes);
  g.dGuideNrm.alloc(bytes);
  if (albedo) g.dGuideAlbedo.alloc(bytes);
  HIP_CHECK(hipMemcpyAsync(g.dCam.p, &C.cam, sizeof(GpuCamera), hipMemcpyHostToDevice, stream));
  evGuides.time(kernelTiming, stream, [&] {
    launch_guides(S.gpu->view, g.dCam.as<GpuCamera>(), W, H, g.dGuidePos.as<float4>(), g.dGuideNrm.as<float4>(),
                  albedo ? g.dGuideAlbedo.as<float4>() : nullptr, stream);
  });
  HIP_CHECK(hipGetLastError());
}

// yrtDenoiseFrameBuffer: guides, c_0 = the frame as it stands, `iterations` a-trous passes
// ping-ponging between two float4 frames, the last one storing into the frame's own format.
// An RGB8 / RGB_FLOAT32 frame still in ctx[0]'s frame block is filtered there (the block holds
// exactly those layouts; the next rtMapFrameBuffer reads the filtered frame back). The RGBA
// formats exist on the host only (fb_read_back converts the block's RGB floats), so such a frame
// is read back first and, like any frame already mapped or rendered into user pointers,
// uploaded from the host pixels, filtered and copied back into them.
// demodulate: the guide pass also renders the first-hit albedo, the load divides the frame by the
// modulation max(albedo, albedoFloor) ^ albedoPower and the last iteration multiplies it back
// (k_atrous<true>); clear, the kernels are the <false> instantiations: no albedo, today's arithmetic.
void Device::denoise(CameraObj& C, SceneObj& S, FrameBufferObj& F, const YRTDenoiseParams& p) {
  if (!S.gpu) throw std::runtime_error("yrtDenoiseFrameBuffer: scene not committed");
  if (p.iterations == 0) return;
  const int W = F.width, H = F.height, id = F.cur;
  if (W < 1 || H < 1) return;
  const bool demod = p.demodulate != 0;
  guides(C, S, W, H, "yrtDenoiseFrameBuffer", demod);
  GpuCtx& g = *ctx[0];
  const bool bytes8 = F.format == FB_RGB8 || F.format == FB_RGBA8;
  const bool rgba = F.format == FB_RGBA8 || F.format == FB_RGBA_FLOAT32;
  FrameIO io;
  io.width = W;
  io.height = H;
  io.pixStride = rgba ? 4 : 3;
  io.bytes = bytes8 ? 1 : 0;
  io.rowStride = bytes8 ? F.stride : F.stride / sizeof(float);
  const bool pending = id < (int)F.pending.size() && F.pending[id].keep;
  const bool inBlock = pending && !rgba && F.pending[id].hipDevice == hipDevice;
  const size_t fbBytes = F.stride * (size_t)H;
  if (inBlock) {
    io.pixels = const_cast<void*>(F.pending[id].src);
  } else {
    if (pending) fb_read_back(F, id);
    HIP_CHECK(hipSetDevice(hipDevice));
    g.dFilterFb.alloc(fbBytes);
    HIP_CHECK(hipMemcpyAsync(g.dFilterFb.p, F.buffer(id), fbBytes, hipMemcpyHostToDevice, stream));
    io.pixels = g.dFilterFb.p;
  }
  const size_t frameBytes = (size_t)W * H * sizeof(float4);
  g.dFilter[0].alloc(frameBytes);
  if (p.iterations > 1) g.dFilter[1].alloc(frameBytes);
  Demodulation dm;
  if (demod) {
    g.dFilterMod.alloc(frameBytes);
    dm.albedo4 = g.dGuideAlbedo.as<float4>();
    dm.mod4 = g.dFilterMod.as<float4>();
    dm.albedoFloor = p.albedoFloor;
    dm.albedoPower = p.albedoPower;
  }
  evFilter.time(kernelTiming, stream, [&] {
    launch_atrous_load(io, g.dFilter[0].as<float4>(), dm, stream);
    AtrousParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.width = W;
    ap.height = H;
    ap.sigmaNormal = p.sigmaNormal;
    ap.sigmaPosition = p.sigmaPosition;
    const FrameIO none{nullptr, 0, W, H, 0, 0};
    for (int i = 0; i < p.iterations; ++i) {
      const bool last = i + 1 == p.iterations;
      ap.step = 1 << i;
      // sigmaColor_i = sigmaColor 2^-i (Dammertz et al.): the colour weight tightens as the taps spread
      const float sc = p.sigmaColor > 0.f ? p.sigmaColor / (float)(1 << i) : 0.f;
      ap.rcpSigmaColor2 = sc > 0.f ? 1.0f / (sc * sc) : 0.f;
      launch_atrous(ap, g.dGuidePos.as<float4>(), g.dGuideNrm.as<float4>(), g.dFilter[i & 1].as<float4>(),
                    last ? nullptr : g.dFilter[(i + 1) & 1].as<float4>(), last ? io : none, dm.mod4, stream);
    }
  });
  HIP_CHECK(hipGetLastError());
  if (!inBlock) HIP_CHECK(hipMemcpyAsync(F.buffer(id), g.dFilterFb.p, fbBytes, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  evGuides.read(msGuides);
  evFilter.read(msFilter);
}

}  // namespace yrt
