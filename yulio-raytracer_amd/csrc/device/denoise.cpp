// denoise.cpp — the denoise stage of the device plugin: the first-hit guide pass (yrtRenderGuides,
// yrtRenderAlbedo) and the edge-avoiding a-trous filter over a rendered frame
// (yrtDenoiseFrameBuffer) or over the faces of a stereo cube as one surface (yrtDenoiseCube).
#include "device.h"

namespace yrt {

// The scene and size checks of the whole stage live here: every entry point comes through.
void Device::guides(const std::vector<CameraObj*>& C, SceneObj& S, int W, int H, const char* what, bool albedo) {
  if (!S.gpu) throw std::runtime_error(std::string(what) + ": scene not committed");
  if (S.gpu->device != hipDevice) throw std::runtime_error(std::string(what) + ": scene committed on another HIP device");
  const int faces = (int)C.size();
  // one thread per pixel in 64-lane blocks: the grid stays far inside 2^31 blocks
  if ((long long)faces * W * H > (1ll << 30)) throw std::runtime_error(std::string(what) + ": more than 2^30 pixels");
  HIP_CHECK(hipSetDevice(hipDevice));
  GpuCtx& g = *ctx[0];
  const size_t bytes = (size_t)faces * W * H * sizeof(float4);
  std::vector<GpuCamera> cams(faces);
  for (int k = 0; k < faces; ++k) cams[k] = C[k]->cam;
  g.dCam.alloc(cams.size() * sizeof(GpuCamera));
  g.dGuidePos.alloc(bytes);
  g.dGuideNrm.alloc(bytes);
  if (albedo) g.dGuideAlbedo.alloc(bytes);
  HIP_CHECK(hipMemcpyAsync(g.dCam.p, cams.data(), cams.size() * sizeof(GpuCamera), hipMemcpyHostToDevice, stream));
  evGuides.time(kernelTiming, stream, [&] {
    launch_guides(S.gpu->view, g.dCam.as<GpuCamera>(), faces, W, H, g.dGuidePos.as<float4>(),
                  g.dGuideNrm.as<float4>(), albedo ? g.dGuideAlbedo.as<float4>() : nullptr, stream);
  });
  HIP_CHECK(hipGetLastError());
}

// Buffer `id` of F as the filter reads and writes it. A frame still pending in this device's frame
// block in the block's own layout (RGB8, RGB_FLOAT32) is filtered there: io.pixels points into the
// block. Any other frame is read back first if it is pending and then lives in F.buffer(id):
// io.pixels is null and the caller uploads it.
Device::FilterFrame Device::filter_frame(FrameBufferObj& F, int id) {
  const bool bytes8 = F.format == FB_RGB8 || F.format == FB_RGBA8;
  const bool rgba = F.format == FB_RGBA8 || F.format == FB_RGBA_FLOAT32;
  FilterFrame ff;
  ff.io.pixels = nullptr;
  ff.io.width = F.width;
  ff.io.height = F.height;
  ff.io.pixStride = rgba ? 4 : 3;
  ff.io.bytes = bytes8 ? 1 : 0;
  ff.io.rowStride = bytes8 ? F.stride : F.stride / sizeof(float);
  const bool pending = id < (int)F.pending.size() && F.pending[id].keep;
  ff.inBlock = pending && !rgba && F.pending[id].hipDevice == hipDevice;
  if (ff.inBlock) ff.io.pixels = const_cast<void*>(F.pending[id].src);
  else if (pending) fb_read_back(F, id);
  return ff;
}

// The sums and half sums the variance of F's displayed frame is estimated from
// (common/yrt_pixel_variance.h): those of F's last render, which must have been an adaptive render
// on ctx[0] in which every tile ran at least two iterations, so that both halves hold samples.
// Judged from host records alone: a refusal launches and writes nothing.
Device::VarianceSource Device::variance_source(FrameBufferObj& F, const char* what) {
  const std::string w(what);
  if (!F.accuFromAdaptive)
    throw std::runtime_error(w + ": the framebuffer's last frame is not an adaptive render (rtRenderAdaptive keeps the "
                                 "half buffer the variance is estimated from)");
  VarianceSource v;
  for (const auto& a : F.accu)
    if (a->ctxSerial == ctx[0]->serial) v.accu = a->sums.as<float4>();
  for (const auto& a : F.adaptive)
    if (a->ctxSerial == ctx[0]->serial) {
      v.half = a->half.as<float4>();
      v.gamma = a->gamma;
      v.rcpGamma = a->rcpGamma;
      v.vignetting = a->vignetting ? 1 : 0;
    }
  if (!v.accu || !v.half)
    throw std::runtime_error(w + ": the framebuffer's adaptive render ran on another device (its sums are not on this one)");
  if (F.tileIterations.empty()) throw std::runtime_error(w + ": the framebuffer has no tile records of an adaptive render");
  for (int32_t n : F.tileIterations)
    if (n < 2)
      throw std::runtime_error(w + ": a tile of the adaptive render ran fewer than 2 iterations (maxIterations 1 or a "
                                   "stop after the first): one half has no samples");
  return v;
}

// yrtFrameVariance: var4 of F's last adaptive render, [H][W][4] floats, to the host
void Device::frame_variance(FrameBufferObj& F, float* var4Host) {
  const VarianceSource v = variance_source(F, "yrtFrameVariance");
  const int W = F.width, H = F.height;
  if (W < 1 || H < 1) return;
  HIP_CHECK(hipSetDevice(hipDevice));
  GpuCtx& g = *ctx[0];
  const size_t bytes = (size_t)W * H * sizeof(float4);
  g.dFilterVar.alloc(bytes);
  launch_frame_variance(v.accu, v.half, W, H, v.gamma, v.rcpGamma, v.vignetting, g.dFilterVar.as<float4>(), stream);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(var4Host, g.dFilterVar.p, bytes, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

// yrtDenoiseFrameBuffer / yrtDenoiseCube: the filter over a surface of C.size() frames of one size
// and format, F[k] seen through C[k]: one frame whose taps stop at its border, or (wrap) the 6 or
// 12 square faces of a stereo cube in slot order k = eye * 6 + cubeFaceIndex % 6, which the caller
// has validated, whose taps cross the cube's edges. Guides, c_0 = the frames as they stand,
// `iterations` a-trous passes ping-ponging between two float4 [face][H][W] arrays, the last one
// storing into the frames' own format, one launch per stage.
// Each frame is filtered where it lives (filter_frame). An RGB8 / RGB_FLOAT32 frame still in
// ctx[0]'s frame block is filtered there (the block holds exactly those layouts; the next
// rtMapFrameBuffer reads the filtered frame back). The RGBA formats exist on the host only
// (fb_read_back converts the block's RGB floats), so such a frame is read back first and, like any
// frame already mapped or rendered into user pointers, uploaded from the host pixels into a
// 16-byte-aligned slot of dFilterFb, filtered and copied back into them.
// demodulate: the guide pass also renders the first-hit albedo, the load divides the frames by the
// modulation max(albedo, albedoFloor) ^ albedoPower and the last iteration multiplies it back
// (k_atrous<true>); clear, the kernels are the <false> instantiations: no albedo.
// varianceGuided: every frame must hold an adaptive render (variance_source, judged before anything
// is launched); k_frame_variance fills a [face][H][W] variance array from each face's own sums and
// half sums, inside the timed filter, and the _var kernels run in place of the plain ones.
void Device::denoise(const std::vector<CameraObj*>& C, SceneObj& S, const std::vector<FrameBufferObj*>& F,
                     const YRTDenoiseParams& p, bool wrap, const char* what) {
  // also of a call that filters nothing (below), which never reaches the guide pass
  if (!S.gpu) throw std::runtime_error(std::string(what) + ": scene not committed");
  const bool variance = p.varianceGuided != 0;
  std::vector<VarianceSource> vs;
  if (variance)
    for (FrameBufferObj* f : F) vs.push_back(variance_source(*f, what));
  if (p.iterations == 0) return;
  const int faces = (int)C.size(), W = F[0]->width, H = F[0]->height;
  if (W < 1 || H < 1) return;
  const bool demod = p.demodulate != 0;
  guides(C, S, W, H, what, demod);
  GpuCtx& g = *ctx[0];

  // the frames: in the block, or uploaded side by side into dFilterFb
  const size_t fbBytes = F[0]->stride * (size_t)H, fbSlot = (fbBytes + 15) / 16 * 16;
  std::vector<FrameIO> ios(faces);
  std::vector<int> ids(faces);
  std::vector<char> onHost(faces, 0);
  size_t uploads = 0;
  for (int k = 0; k < faces; ++k) {
    ids[k] = F[k]->cur;
    const FilterFrame ff = filter_frame(*F[k], ids[k]);
    ios[k] = ff.io;
    if (!ff.inBlock) {
      onHost[k] = 1;
      ++uploads;
    }
  }
  HIP_CHECK(hipSetDevice(hipDevice));  // a read-back may have selected the frame's device
  if (uploads) {
    g.dFilterFb.alloc(uploads * fbSlot);
    size_t u = 0;
    for (int k = 0; k < faces; ++k) {
      if (!onHost[k]) continue;
      ios[k].pixels = (char*)g.dFilterFb.p + u++ * fbSlot;
      HIP_CHECK(hipMemcpyAsync(ios[k].pixels, F[k]->buffer(ids[k]), fbBytes, hipMemcpyHostToDevice, stream));
    }
  }
  g.dFaceIo.alloc(ios.size() * sizeof(FrameIO));
  HIP_CHECK(hipMemcpyAsync(g.dFaceIo.p, ios.data(), ios.size() * sizeof(FrameIO), hipMemcpyHostToDevice, stream));
  const size_t frameBytes = (size_t)faces * W * H * sizeof(float4);
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
  if (variance) g.dFilterVar.alloc(frameBytes);
  evFilter.time(kernelTiming, stream, [&] {
    if (variance) {
      for (int k = 0; k < faces; ++k)
        launch_frame_variance(vs[k].accu, vs[k].half, W, H, vs[k].gamma, vs[k].rcpGamma, vs[k].vignetting,
                              g.dFilterVar.as<float4>() + (size_t)k * W * H, stream);
      launch_atrous_load_var(g.dFaceIo.as<FrameIO>(), faces, W, H, g.dFilter[0].as<float4>(), dm,
                             g.dFilterVar.as<float4>(), g.dGuidePos.as<float4>(), stream);
    } else {
      launch_atrous_load(g.dFaceIo.as<FrameIO>(), faces, W, H, g.dFilter[0].as<float4>(), dm, stream);
    }
    AtrousParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.width = W;
    ap.height = H;
    ap.sigmaNormal = p.sigmaNormal;
    ap.sigmaPosition = p.sigmaPosition;
    for (int i = 0; i < p.iterations; ++i) {
      const bool last = i + 1 == p.iterations;
      ap.step = 1 << i;
      // sigmaColor_i = sigmaColor 2^-i (Dammertz et al.): the colour weight tightens as the taps spread
      const float sc = p.sigmaColor > 0.f ? p.sigmaColor / (float)(1 << i) : 0.f;
      ap.rcpSigmaColor2 = sc > 0.f ? 1.0f / (sc * sc) : 0.f;
      if (variance)  // no 2^-i tightening: the filtered variance itself shrinks
        launch_atrous_var(ap, faces, wrap, g.dGuidePos.as<float4>(), g.dGuideNrm.as<float4>(),
                          g.dFilter[i & 1].as<float4>(), last ? nullptr : g.dFilter[(i + 1) & 1].as<float4>(),
                          last ? g.dFaceIo.as<FrameIO>() : nullptr, dm.mod4, p.sigmaVariance * p.sigmaVariance,
                          p.varianceFloor, stream);
      else
        launch_atrous(ap, faces, wrap, g.dGuidePos.as<float4>(), g.dGuideNrm.as<float4>(),
                      g.dFilter[i & 1].as<float4>(), last ? nullptr : g.dFilter[(i + 1) & 1].as<float4>(),
                      last ? g.dFaceIo.as<FrameIO>() : nullptr, dm.mod4, stream);
    }
  });
  HIP_CHECK(hipGetLastError());
  for (int k = 0; k < faces; ++k)
    if (onHost[k])
      HIP_CHECK(hipMemcpyAsync(F[k]->buffer(ids[k]), ios[k].pixels, fbBytes, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  evGuides.read(msGuides);
  evFilter.read(msFilter);
}

// The ideal cube's rotation of face 0 that gives face f, in face 0's own frame (x right, y up,
// z forward): StereoCubeCamera turns faces 1..3 about `up` by 90, 180 and -90 degrees and faces
// 4 / 5 about `right` by -90 / 90 degrees and then about `up` by 180. These are the rotations the
// adjacency table of yrt_cube_tap.h follows.
static const int kCubeRotation[6][3][3] = {
    {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}},   {{0, 0, 1}, {0, 1, 0}, {-1, 0, 0}},  {{-1, 0, 0}, {0, 1, 0}, {0, 0, -1}},
    {{0, 0, -1}, {0, 1, 0}, {1, 0, 0}},  {{-1, 0, 0}, {0, 0, 1}, {0, 1, 0}},  {{-1, 0, 0}, {0, 0, -1}, {0, -1, 0}},
};

// Do the six pixel2world frames of a stereo camera tile the sphere as the ideal cube does? Face
// 0's frame must be a 90-degree square frustum (dir = px vx + (1 - py) vy + vz: vx, vy and
// 2 vz + vx + vy orthogonal and of one length) and face f's linear part that frame turned by
// kCubeRotation[f], to 1e-4 of the frame's length per entry (about 100 times the float rounding of
// the reference's construction, far below a pixel at any supported size). A lookAt that is not
// perpendicular to `up` fails: the reference then turns the faces about axes that are not the
// frame's own. Empty: yes; otherwise what is wrong.
std::string cube_cameras_defect(const GpuCamera& cam) {
  const float* p0 = cam.p2w[0];
  double Bm[3][3];  // columns X, Y, Z as Bm[row][col]
  for (int r = 0; r < 3; ++r) {
    Bm[r][0] = p0[r];
    Bm[r][1] = p0[3 + r];
    Bm[r][2] = 2.0 * p0[6 + r] + p0[r] + p0[3 + r];
  }
  double len[3], dots[3];
  for (int c = 0; c < 3; ++c) len[c] = std::sqrt(Bm[0][c] * Bm[0][c] + Bm[1][c] * Bm[1][c] + Bm[2][c] * Bm[2][c]);
  const double s = len[0];
  if (!(s > 0.0) || !std::isfinite(s)) return "face 0's pixel2world frame is degenerate";
  const double tol = 1e-4;
  const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (int k = 0; k < 3; ++k) {
    const int a = pairs[k][0], b = pairs[k][1];
    dots[k] = (Bm[0][a] * Bm[0][b] + Bm[1][a] * Bm[1][b] + Bm[2][a] * Bm[2][b]) / (s * s);
  }
  if (std::fabs(len[1] / s - 1) > tol || std::fabs(len[2] / s - 1) > tol || std::fabs(dots[0]) > tol ||
      std::fabs(dots[1]) > tol || std::fabs(dots[2]) > tol)
    return "face 0 is not a square 90-degree view (its pixel2world axes are not orthogonal and of one length)";
  // C: (px, 1 - py, 1) -> the direction's coordinates in (X, Y, Z)
  const double Cm[3][3] = {{1, 0, -0.5}, {0, 1, -0.5}, {0, 0, 0.5}};
  for (int f = 1; f < 6; ++f) {
    double MC[3][3], want[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        MC[r][c] = 0;
        for (int k = 0; k < 3; ++k) MC[r][c] += kCubeRotation[f][r][k] * Cm[k][c];
      }
    double worst = 0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        want[r][c] = 0;
        for (int k = 0; k < 3; ++k) want[r][c] += Bm[r][k] * MC[k][c];
        worst = std::max(worst, std::fabs(cam.p2w[f][3 * c + r] - want[r][c]) / s);
      }
    if (!(worst <= tol)) {
      char buf[256];
      snprintf(buf, sizeof(buf),
               "the cameras do not form a cube: face %d is not face 0 turned by the cube's rotation (deviation %.3g of "
               "the frame, tolerance 1e-4); lookAt - origin must be perpendicular to up",
               f, worst);
      return buf;
    }
  }
  return "";
}

}  // namespace yrt
