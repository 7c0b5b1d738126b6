// api_tools.cpp — the C-ABI entry points (include/yrt_device.h) beyond the reference's Device
// virtuals: render statistics, tunables, BVH and frame export, the debug probes, tile shards,
// the shard communicator and the in-process hub.
#include <strings.h>

#include "../common/yrt_cube_tap.h"
#include "../common/yrt_tile_error.h"
#include "../common/yrt_tile_scatter.h"
#include "device.h"
#include "image_io.h"
#include "render_job.h"

using namespace yrt;

extern "C" {

int yrtGetRenderStats(YRTDevice dev, YRTRenderStats* out) {
  DEV_GUARD(dev, -1)
  *out = dev->d->stats;
  return 0;
  DEV_END(-1)
}
int yrtSetKernelTiming(YRTDevice dev, int enable) {
  DEV_GUARD(dev, -1)
  dev->d->kernelTiming = enable != 0;
  return 0;
  DEV_END(-1)
}
int yrtSetLanes(YRTDevice dev, int lanes) {
  DEV_GUARD(dev, -1)
  if (lanes < 0 || lanes > GpuCtx::kMaxLanes)
    throw std::runtime_error("yrtSetLanes: 1.." + std::to_string(GpuCtx::kMaxLanes) + " lanes (YRT_MAX_LANES), 0 = default");
  for (auto& c : dev->d->ctx) c->numLanes = lanes ? lanes : GpuCtx::default_lanes();
  return 0;
  DEV_END(-1)
}
int yrtGetSceneInfo(YRTDevice dev, YRTHandle scene, YRTSceneInfo* out) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S->gpu) throw std::runtime_error("scene not committed");
  out->numTriangles = S->gpu->numTris;
  out->numGeometries = S->gpu->numGeoms;
  out->numNodes = (int64_t)S->gpu->hNodes.size();
  out->numTriRefs = (int64_t)S->gpu->hTris.size();
  out->triRecordBytes = (int64_t)sizeof(GpuTri);
  out->nodeBytesClosest = out->nodeBytesAny = (int)sizeof(GpuQNode);  // k_trace reads the quantized nodes only
  out->bvhDepth = S->gpu->bvhDepth;
  out->numLights = S->gpu->view.numLights;
  out->buildSeconds = S->gpu->buildSeconds;
  for (int k = 0; k < 3; ++k) { out->bboxLo[k] = S->gpu->bboxLo[k]; out->bboxHi[k] = S->gpu->bboxHi[k]; }
  return 0;
  DEV_END(-1)
}
int yrtGetSceneBuildInfo(YRTDevice dev, YRTHandle scene, YRTSceneBuildInfo* out) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S->gpu) throw std::runtime_error("scene not committed");
  if (!out || out->size < sizeof(out->size)) throw std::runtime_error("yrtGetSceneBuildInfo: size not set");
  const BuildInfo& b = S->gpu->buildInfo;
  YRTSceneBuildInfo r;
  memset(&r, 0, sizeof(r));
  r.size = out->size;
  r.builder = b.builder;
  r.fallback = b.fallback;
  r.msBuild = b.msBuild;
  r.msKernels = b.msKernels;
  r.sahCost = b.sahCost;
  memcpy(out, &r, std::min((size_t)out->size, sizeof(r)));  // never past the caller's struct
  return 0;
  DEV_END(-1)
}
int yrtExportBVH(YRTDevice dev, YRTHandle scene, void* nodes, size_t nodesBytes, void* tris, size_t trisBytes) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S->gpu) throw std::runtime_error("scene not committed");
  sync_host_bvh(*S->gpu);
  const size_t nb = S->gpu->hNodes.size() * sizeof(GpuNode), tb = S->gpu->hTris.size() * sizeof(GpuTri);
  if (nodesBytes < nb || trisBytes < tb) throw std::runtime_error("buffers too small");
  memcpy(nodes, S->gpu->hNodes.data(), nb);
  memcpy(tris, S->gpu->hTris.data(), tb);
  return 0;
  DEV_END(-1)
}
int yrtExportQuantizedBVH(YRTDevice dev, YRTHandle scene, void* qnodes, size_t qnodesBytes) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S->gpu) throw std::runtime_error("scene not committed");
  sync_host_bvh(*S->gpu);
  const size_t nb = S->gpu->hQNodes.size() * sizeof(GpuQNode);
  if (qnodesBytes < nb) throw std::runtime_error("buffer too small");
  memcpy(qnodes, S->gpu->hQNodes.data(), nb);
  return 0;
  DEV_END(-1)
}
int yrtSetFrameSeed(YRTDevice dev, uint32_t seed) {
  DEV_GUARD(dev, -1)
  dev->d->frameSeed = seed;
  return 0;
  DEV_END(-1)
}
int yrtSetBatchCapacity(YRTDevice dev, int64_t paths) {
  DEV_GUARD(dev, -1)
  if (paths < 256) throw std::runtime_error("capacity must be >= 256 paths");
  dev->d->capacity = paths;
  return 0;
  DEV_END(-1)
}
int64_t yrt_export_frame_impl(const Object* renderer, const Object* camera, const SceneObj* scene, uint32_t frameSeed,
                              void* buf, size_t bytes);
int64_t yrtExportFrame(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene, void* buf, size_t bytes) {
  DEV_GUARD(dev, -1)
  auto R = dev->d->get<RendererObj>(renderer, "renderer");
  auto C = dev->d->get<CameraObj>(camera, "camera");
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!R || !C || !S) throw std::runtime_error("yrtExportFrame: null handle");
  return yrt_export_frame_impl(R.get(), C.get(), S.get(), dev->d->frameSeed, buf, bytes);
  DEV_END(-1)
}

int yrtDebugSampleTable(int spp, int sets, int iteration, int num1D, int num2D, const char* filter, float* out,
                        size_t outFloats) {
  try {
    SampleRequest req;
    req.spp = spp;
    req.sets = sets;
    req.iteration = iteration;
    req.num1D = num1D;
    req.num2D = num2D;
    req.filter = filter ? filter : "bspline";
    SampleTable t;
    build_sample_table(req, t);
    if (out && outFloats >= t.dims.size()) memcpy(out, t.dims.data(), t.dims.size() * sizeof(float));
    return t.numRecords;
  } catch (...) {
    return -1;
  }
}

int yrtDebugDecodeImage(const char* file, int* width, int* height, int* channels, uint8_t* out, size_t outBytes) {
  try {
    FILE* f = fopen(file, "rb");
    if (!f) return -1;
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    fclose(f);
    std::string err;
    std::vector<uint8_t> px;
    int w = 0, h = 0, c = 3;
    const char* dot = strrchr(file, '.');
    if (dot && (!strcasecmp(dot, ".jpg") || !strcasecmp(dot, ".jpeg"))) {
      if (!decode_jpeg(bytes, w, h, px, err)) return -2;
    } else if (dot && !strcasecmp(dot, ".png")) {
      if (!decode_png(bytes, w, h, c, px, err)) return -2;
    } else {
      return -3;
    }
    *width = w;
    *height = h;
    *channels = c;
    if (out && outBytes >= px.size()) memcpy(out, px.data(), px.size());
    return 0;
  } catch (...) {
    return -4;
  }
}

int yrtSetRayCapture(YRTDevice dev, int maxPerDepth) {
  DEV_GUARD(dev, -1)
  dev->d->captureMax = std::max(0, maxPerDepth);
  return 0;
  DEV_END(-1)
}

int64_t yrtGetCapturedRays(YRTDevice dev, int shadow, int depth, float* org4, float* dir4, size_t maxRays,
                           double* totalInBatch) {
  DEV_GUARD(dev, -1)
  if (dev->d->ctx.empty()) throw std::runtime_error("host-only device");
  auto& v = shadow ? dev->d->ctx[0]->capShadow : dev->d->ctx[0]->capClosest;
  if (depth < 0 || depth >= (int)v.size()) {
    if (totalInBatch) *totalInBatch = 0;
    return 0;
  }
  const auto& c = v[depth];
  const size_t m = c.org.size() / 4;
  if (totalInBatch) *totalInBatch = c.total;
  if (org4 && dir4) {
    const size_t k = std::min(m, maxRays);
    memcpy(org4, c.org.data(), k * 16);
    memcpy(dir4, c.dir.data(), k * 16);
  }
  return (int64_t)m;
  DEV_END(-1)
}

int yrtDebugTraceProfile(YRTDevice dev, uint64_t* out8, int reset) {
  DEV_GUARD(dev, -1)
  HIP_CHECK(hipDeviceSynchronize());
  return trace_profile((unsigned long long*)out8, reset);
  DEV_END(-1)
}

int yrtDebugPixelSamples(YRTDevice dev, int pixelId, int frame, float* out4, int maxSamples) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("host-only device");
  HIP_CHECK(hipSetDevice(D.hipDevice));
  // one capture at a time per process (the kernel-side target is a module global)
  DevBuf& buf = D.dbgPixelBuf;
  if (!out4) {
    if (pixelId < 0) return debug_pixel_capture(-1, -1, nullptr, 0);
    if (maxSamples < 1) throw std::runtime_error("yrtDebugPixelSamples: maxSamples < 1");
    buf.alloc((size_t)maxSamples * sizeof(float4));
    HIP_CHECK(hipMemset(buf.p, 0, (size_t)maxSamples * sizeof(float4)));
    D.dbgPixelCap = maxSamples;
    return debug_pixel_capture(pixelId, frame, buf.as<float4>(), maxSamples);
  }
  if (!buf.p) throw std::runtime_error("yrtDebugPixelSamples: no capture armed on this device");
  const int n = std::min(maxSamples, D.dbgPixelCap);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(out4, buf.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
  return n;
  DEV_END(-1)
}

int yrtDebugCheckMath(YRTDevice dev, int fn, uint64_t* out2) {
  DEV_GUARD(dev, -1)
  if ((fn != 0 && fn != 3 && fn != 4) || !out2) throw std::runtime_error("yrtDebugCheckMath: fn 0, 3 or 4");
  HIP_CHECK(hipSetDevice(dev->d->hipDevice));
  if (check_math(fn, (unsigned long long*)out2) != 0) throw std::runtime_error("check_math failed");
  return 0;
  DEV_END(-1)
}

int yrtDebugCheckMathTable(YRTDevice dev, int fn, const uint16_t* table2048, uint64_t* out2) {
  DEV_GUARD(dev, -1)
  if ((fn != 1 && fn != 2) || !table2048 || !out2) throw std::runtime_error("yrtDebugCheckMathTable: fn 1 or 2");
  HIP_CHECK(hipSetDevice(dev->d->hipDevice));
  if (check_math_table(fn, table2048, (unsigned long long*)out2) != 0) throw std::runtime_error("check_math_table failed");
  return 0;
  DEV_END(-1)
}

int yrtDebugSampleDirs(YRTDevice dev, int spp, int sets, int iteration, int num1D, int num2D, const char* filter,
                       float* dims, size_t dimsFloats, float* dirs4, size_t dirsFloats) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("yrtDebugSampleDirs: host-only device");
  if (spp < 1 || sets < 1 || iteration < 0 || num1D < 0 || num2D < 0)
    throw std::runtime_error("yrtDebugSampleDirs: invalid arguments");
  HIP_CHECK(hipSetDevice(D.ctx[0]->hipDevice));
  SampleRequest req;
  req.spp = spp;
  req.sets = sets;
  req.iteration = iteration;
  req.num1D = num1D;
  req.num2D = num2D;
  req.filter = filter ? filter : "bspline";
  const FrameCache& fc = frame_cache(*D.ctx[0], req, 0);
  const SampleTable& t = fc.table;
  const size_t nd = (size_t)num2D * t.numRecords * 4;
  if (dims && dimsFloats >= t.dims.size()) memcpy(dims, t.dims.data(), t.dims.size() * sizeof(float));
  if (dirs4 && nd && dirsFloats >= nd) HIP_CHECK(hipMemcpy(dirs4, fc.dirs.p, nd * sizeof(float), hipMemcpyDeviceToHost));
  return t.numRecords;
  DEV_END(-1)
}

int yrtDebugDirTerms(YRTDevice dev, int mode, const float* u, const float* v, int n, float* out4) {
  DEV_GUARD(dev, -1)
  if (!dev->d->gpu) throw std::runtime_error("yrtDebugDirTerms: host-only device");
  HIP_CHECK(hipSetDevice(dev->d->hipDevice));
  if (check_dir_terms(mode, n, u, v, out4) != 0) throw std::runtime_error("yrtDebugDirTerms: invalid arguments or HIP error");
  return 0;
  DEV_END(-1)
}

int yrtDebugShade(YRTDevice dev, int mode, YRTHandle object, const float* rows, int n, const void* materials,
                  int numMaterials, float* out) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("yrtDebugShade: host-only device");
  if (mode < 0 || mode > 3 || !rows || !out || n < 1) throw std::runtime_error("yrtDebugShade: invalid arguments");
  const GpuCamera* cam = nullptr;
  GpuLight light;
  const GpuLight* lp = nullptr;
  if (mode == 2) {
    auto C = D.get<CameraObj>(object, "camera");
    if (!C) throw std::runtime_error("yrtDebugShade: mode 2 takes a committed camera");
    cam = &C->cam;
  } else if (mode == 3) {
    auto P = D.get<PrimitiveObj>(object, "primitive");
    if (!P || !P->lightHandle || !P->lightHandle->inst)
      throw std::runtime_error("yrtDebugShade: mode 3 takes a primitive of a committed light");
    // the world-space light rtSetPrimitive would place in a scene
    light = gpu_light_record(*P->lightHandle->inst->transform(P->transform, P->illumMask, P->shadowMask));
    lp = &light;
  }
  HIP_CHECK(hipSetDevice(D.hipDevice));
  if (check_shade(mode, n, rows, (const GpuMaterial*)materials, numMaterials, cam, lp, out) != 0)
    throw std::runtime_error("yrtDebugShade: invalid rows or a failed launch");
  return 0;
  DEV_END(-1)
}

int yrtDebugMaterial(YRTDevice dev, YRTHandle scene, YRTHandle primitive, int mode, const char* set,
                     const float* medium4, const float* rows, int n, float* out) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("yrtDebugMaterial: host-only device");
  if ((mode != 0 && mode != 1) || !rows || !out || n < 1 || (mode == 0 && !medium4))
    throw std::runtime_error("yrtDebugMaterial: invalid arguments");
  auto S = D.get<SceneObj>(scene, "scene");
  auto P = D.get<PrimitiveObj>(primitive, "primitive");
  if (!S || !S->gpu || !P) throw std::runtime_error("yrtDebugMaterial: takes a committed scene and one of its primitives");
  const GpuScene& G = *S->gpu;
  // the primitive's geometry among the slots the scene was committed with
  int geom = -1;
  for (size_t i = 0; i < G.slotsCommitted.size() && i < G.slotGeom.size() && geom < 0; ++i)
    if (G.slotsCommitted[i] && G.slotsCommitted[i]->prim == P) geom = G.slotGeom[i];
  if (geom < 0 || geom >= (int)G.hGeoms.size())
    throw std::runtime_error("yrtDebugMaterial: the primitive is no shape of the committed scene");
  const int mat = G.hGeoms[geom].material;
  if (mat < 0 || mat >= (int)G.hMaterials.size()) throw std::runtime_error("yrtDebugMaterial: the primitive has no material");
  // every index the kernels follow from the record: the texture ids and their images
  for (int k = 0; k < 5; ++k) {
    const int t = G.hMaterials[mat].tex[k];
    if (t >= (int)G.hTextures.size() || (t >= 0 && (G.hTextures[t].image < 0 || G.hTextures[t].image >= (int)G.hImages.size())))
      throw std::runtime_error("yrtDebugMaterial: texture id out of range");
  }
  const int variant = shade_variant_index(set);
  if (variant < 0) throw std::runtime_error(std::string("yrtDebugMaterial: unknown material set '") + (set ? set : "") + "'");
  int medium = 0;
  if (mode == 0) {  // Medium::operator== compares by value; a medium the scene does not hold equals none of its own
    medium = (int)G.hMedia.size();
    for (size_t i = 0; i < G.hMedia.size() && medium == (int)G.hMedia.size(); ++i)
      if (G.hMedia[i].x == medium4[0] && G.hMedia[i].y == medium4[1] && G.hMedia[i].z == medium4[2] &&
          G.hMedia[i].w == medium4[3])
        medium = (int)i;
  }
  HIP_CHECK(hipSetDevice(G.device));
  const int rc = check_material(G.view, mode, variant, G.hMaterials[mat].type, geom, medium, n, rows, out);
  if (rc == -2) throw std::runtime_error(std::string("yrtDebugMaterial: the material set '") + set + "' does not hold the primitive's material");
  if (rc != 0) throw std::runtime_error("yrtDebugMaterial: a failed launch");
  return 0;
  DEV_END(-1)
}

int64_t yrtDebugTexturePool(YRTDevice dev, YRTHandle scene, int what, void* buf, size_t bytes) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S || !S->gpu) throw std::runtime_error("scene not committed");
  const GpuScene& G = *S->gpu;
  const bool host = !dev->d->gpu;
  std::vector<uint32_t> quads;
  const void* src = nullptr;   // host memory
  const void* dsrc = nullptr;  // device memory
  size_t n = 0;
  switch (what) {
    case 0: src = G.hImages.data(); n = G.hImages.size() * sizeof(GpuImage); break;
    case 1: src = G.hTextures.data(); n = G.hTextures.size() * sizeof(GpuTexture); break;
    case 2: n = G.texelsBytes; if (host) src = G.hTexels.data(); else dsrc = G.texels.p; break;
    case 3:
      n = 4 * G.texels8Bytes;
      if (!host) dsrc = G.texQuads.p;
      else if (buf && bytes >= n) { quads = build_tex_quads(G.hImages, G.hTexels, G.texels8Bytes); src = quads.data(); }
      break;
    default: throw std::runtime_error("yrtDebugTexturePool: what 0..3");
  }
  if (buf && bytes >= n && n) {
    if (dsrc) {
      HIP_CHECK(hipSetDevice(G.device));
      HIP_CHECK(hipMemcpy(buf, dsrc, n, hipMemcpyDeviceToHost));
    } else {
      memcpy(buf, src, n);
    }
  }
  return (int64_t)n;
  DEV_END(-1)
}

int yrtDebugTileScatter(int t, int T) {
  if (T < 1 || t < 0 || t >= T) return -1;
  return yrt_tile_scatter(t, T);
}

int yrtDebugTileSlab(YRTDevice dev, int width, int height, int numFrames, int rgb8, int tileOffset, int tileStride,
                     int numTiles, int op, float* fbFloat, size_t fbFloatBytes, uint8_t* fbRGB8, size_t fbRGB8Bytes,
                     void* slab, size_t slabBytes) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (width < 1 || height < 1 || numFrames < 1 || width > (1 << 20) || height > (1 << 20) || numTiles < 0 ||
      tileStride < 1 || tileOffset < 0 || (op != 0 && op != 1) || !fbFloat || !fbRGB8 || !slab)
    throw std::runtime_error("yrtDebugTileSlab: invalid arguments");
  const int64_t tilesPerFrame = (int64_t)((width + 15) / 16) * ((height + 15) / 16);
  const int64_t total = tilesPerFrame * numFrames;
  if (total * 256 > INT32_MAX)
    throw std::runtime_error("yrtDebugTileSlab: the job's pixels do not fit the kernels' int index");
  // numTiles <= shard_tiles(total, tileOffset, tileStride), in 64 bits (any stride): the last
  // tile the kernels address, tileOffset + (numTiles - 1) * tileStride, is a tile of the job
  if (numTiles > 0 && (int64_t)tileOffset + (int64_t)(numTiles - 1) * tileStride >= total)
    throw std::runtime_error("yrtDebugTileSlab: numTiles exceeds the shard's tiles");
  const size_t floatBytes = (size_t)numFrames * height * width * 3 * sizeof(float);
  const size_t rgb8Bytes = GpuCtx::FrameBlock::rgb8_bytes(width, height, numFrames);
  const size_t needSlab = (size_t)numTiles * 256 * slab_element_bytes(rgb8 ? 1 : 0);
  if (fbFloatBytes < floatBytes || fbRGB8Bytes < rgb8Bytes || slabBytes < needSlab)
    throw std::runtime_error("yrtDebugTileSlab: a host buffer is smaller than the job");
  const SlabLayout L{width, height, (int)rgb8_row_stride(width), (int)tilesPerFrame, tileOffset, tileStride,
                     rgb8 ? 1 : 0, 0};
  // the arguments are judged first, so a host-only device refuses the invalid ones for their own reason
  if (!D.gpu) throw std::runtime_error("yrtDebugTileSlab: host-only device");
  HIP_CHECK(hipSetDevice(D.hipDevice));
  DevBuf dF, dB, dS;
  dF.alloc(floatBytes);
  dB.alloc(rgb8Bytes);
  dS.alloc(slabBytes);  // the caller's whole slab travels: what lies behind the shard's elements returns as it went
  HIP_CHECK(hipMemcpy(dF.p, fbFloat, floatBytes, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB.p, fbRGB8, rgb8Bytes, hipMemcpyHostToDevice));
  if (slabBytes) HIP_CHECK(hipMemcpy(dS.p, slab, slabBytes, hipMemcpyHostToDevice));
  if (op == 0) {
    launch_pack_tiles(dF.as<float>(), dB.as<uint8_t>(), L, numTiles, dS.p, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (slabBytes) HIP_CHECK(hipMemcpy(slab, dS.p, slabBytes, hipMemcpyDeviceToHost));
  } else {
    launch_unpack_tiles(dS.p, dF.as<float>(), dB.as<uint8_t>(), L, numTiles, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(fbFloat, dF.p, floatBytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(fbRGB8, dB.p, rgb8Bytes, hipMemcpyDeviceToHost));
  }
  return 0;
  DEV_END(-1)
}

int yrtDebugCubeTap(int W, int face, int qx, int qy, int* g, int* x, int* y) {
  if (!g || !x || !y) return -1;
  return yrt_cube_tap(W, face, qx, qy, g, x, y);
}

int yrtDebugBatchPlan(int64_t shardTiles, int spp, int64_t capacity, int lanes, int capture, int grow, int64_t* out4) {
  if (shardTiles < 0 || spp < 1 || capacity < 1 || lanes < 1 || !out4) return -1;
  const BatchPlan p = plan_batches(shardTiles, spp, capacity, lanes, capture != 0, grow != 0);
  out4[0] = p.tilesPerBatch;
  out4[1] = p.numBatches;
  out4[2] = p.pathsPerBatch;
  out4[3] = p.lanes;
  return 0;
}

int yrtSetTileShard(YRTDevice dev, int index, int count) {
  DEV_GUARD(dev, -1)
  if (count < 1 || index < 0 || index >= count) throw std::runtime_error("invalid shard");
  // a process communicator gathers exactly its own shard (rank of world): another shard would
  // post sends/receives its peers never match
  if (dev->d->proc && (index != dev->d->commRank || count != dev->d->commWorld))
    throw std::runtime_error("yrtSetTileShard: shard differs from the process communicator's (rank " +
                             std::to_string(dev->d->commRank) + " of " + std::to_string(dev->d->commWorld) +
                             "); call yrtSetShardComm(dev, 0, 1, id) or yrtSetShardHub(dev, NULL, 0) first to drop it");
  dev->d->shardIndex = index;
  dev->d->shardCount = count;
  return 0;
  DEV_END(-1)
}

int yrtRcclAvailable(void) {
  try {
    (void)rccl();
    return 1;
  } catch (...) {
    return 0;
  }
}

int yrtShardCommUniqueId(void* id128) {
  try {
    ncclUniqueId id;
    rccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
    memcpy(id128, &id, sizeof(id));
    return 0;
  } catch (...) {
    return -1;
  }
}

int yrtSetShardComm(YRTDevice dev, int rank, int world, const void* id128) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (world < 1 || rank < 0 || rank >= world) throw std::runtime_error("invalid shard");
  if (!D.gpu) throw std::runtime_error("host-only device");
  HIP_CHECK(hipSetDevice(D.hipDevice));
  D.proc.reset();
  D.commRank = 0;
  D.commWorld = 1;
  if (world > 1) {
    D.proc = make_rccl_transport(rank, world, id128);
    D.commRank = rank;
    D.commWorld = world;
  }
  D.shardIndex = rank;
  D.shardCount = world;
  return 0;
  DEV_END(-1)
}

struct YRTShardHub_ {
  std::shared_ptr<ShardHub> hub;
};
static thread_local std::string t_hubError;

YRTShardHub yrtNewShardHub(int world) {
  try {
    auto* h = new YRTShardHub_;
    h->hub = make_shard_hub(world);
    return h;
  } catch (const std::exception& e) {
    t_hubError = e.what();
    return nullptr;
  }
}

void yrtDeleteShardHub(YRTShardHub hub) { delete hub; }

int yrtSetShardHub(YRTDevice dev, YRTShardHub hub, int rank) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  D.proc.reset();
  D.commRank = 0;
  D.commWorld = 1;
  D.shardIndex = 0;
  D.shardCount = 1;
  if (!hub) return 0;
  const int world = shard_hub_world(*hub->hub);
  if (rank < 0 || rank >= world) throw std::runtime_error("yrtSetShardHub: invalid rank");
  if (!D.gpu && world > 1) throw std::runtime_error("host-only device");
  if (world > 1) {
    D.proc = make_hub_transport(hub->hub, rank);
    D.commRank = rank;
    D.commWorld = world;
  }
  D.shardIndex = rank;
  D.shardCount = world;
  return 0;
  DEV_END(-1)
}

int yrtSetGatherTimeout(YRTDevice dev, double seconds) {
  DEV_GUARD(dev, -1)
  if (!(seconds > 0)) throw std::runtime_error("yrtSetGatherTimeout: seconds must be > 0");
  dev->d->gatherTimeout = seconds;
  return 0;
  DEV_END(-1)
}

int yrtShardHubStatus(YRTShardHub hub, int rank, int flag, double timeoutS) {
  try {
    if (!hub) throw std::runtime_error("null hub");
    return hub_host_status(*hub->hub, rank, flag, timeoutS);
  } catch (const std::exception& e) {
    t_hubError = e.what();
    return -1;
  }
}

int yrtShardHubSlab(YRTShardHub hub, int rank, const void* slab, size_t bytes, void* recv, size_t recvBytesPerRank,
                    double timeoutS) {
  try {
    if (!hub) throw std::runtime_error("null hub");
    hub_host_slab(*hub->hub, rank, slab, bytes, recv, recvBytesPerRank, timeoutS);
    return 0;
  } catch (const std::exception& e) {
    t_hubError = e.what();
    return -1;
  }
}

const char* yrtShardHubLastError(void) { return t_hubError.c_str(); }

int yrtGetDeviceCount(YRTDevice dev) {
  DEV_GUARD(dev, -1)
  return (int)dev->d->ctx.size();
  DEV_END(-1)
}

int yrtSetRefitCommits(YRTDevice dev, int on) {
  DEV_GUARD(dev, -1)
  dev->d->refitCommits = on != 0;
  return 0;
  DEV_END(-1)
}

int yrtGetSceneRefits(YRTDevice dev, YRTHandle scene) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S || !S->gpu) throw std::runtime_error("scene not committed");
  return S->gpu->refits;
  DEV_END(-1)
}

// The library's YRTAdaptiveParams: the defaults overlaid by the fields the caller's struct holds
// (the convention of YRTDenoiseParams). The values are judged by Device::render_adaptive.
static YRTAdaptiveParams adaptive_params(const YRTAdaptiveParams* p) {
  YRTAdaptiveParams d;
  d.size = (uint32_t)sizeof(YRTAdaptiveParams);
  d.threshold = 0.05f;
  d.minIterations = 2;
  d.maxIterations = 64;
  if (!p) return d;
  if (p->size < sizeof(uint32_t)) throw std::runtime_error("YRTAdaptiveParams: size is smaller than the size field");
  const size_t n = p->size;
#define YRT_AD_FIELD(f) \
  if (n >= offsetof(YRTAdaptiveParams, f) + sizeof(d.f)) d.f = p->f
  YRT_AD_FIELD(threshold);
  YRT_AD_FIELD(minIterations);
  YRT_AD_FIELD(maxIterations);
#undef YRT_AD_FIELD
  return d;
}

int yrtAdaptiveDefaults(YRTAdaptiveParams* p) {
  if (!p || p->size < sizeof(uint32_t)) return -1;
  const YRTAdaptiveParams d = adaptive_params(nullptr);
  memcpy((char*)p + sizeof(uint32_t), (const char*)&d + sizeof(uint32_t),
         std::min<size_t>(p->size, sizeof(d)) - sizeof(uint32_t));
  return 0;
}

int yrtRenderAdaptive(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene, YRTHandle tonemapper,
                      YRTHandle framebuffer, const YRTAdaptiveParams* p, YRTAdaptiveStats* out) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  auto R = D.get<RendererObj>(renderer, "renderer");
  auto C = D.get<CameraObj>(camera, "camera");
  auto S = D.get<SceneObj>(scene, "scene");
  auto T = D.get<ToneMapperObj>(tonemapper, "tonemapper");
  auto F = D.get<FrameBufferObj>(framebuffer, "framebuffer");
  if (!R || !C || !S || !T || !F) throw std::runtime_error("rtRenderAdaptive: null handle");
  if (out && out->size < sizeof(uint32_t)) throw std::runtime_error("YRTAdaptiveStats: size not set");
  YRTAdaptiveStats r;
  memset(&r, 0, sizeof(r));
  D.render_adaptive(*R, *C, *S, *T, *F, adaptive_params(p), r);
  if (out) {
    r.size = out->size;
    memcpy(out, &r, std::min((size_t)out->size, sizeof(r)));  // never past the caller's struct
  }
  return 0;
  DEV_END(-1)
}

int yrtGetAdaptiveTiles(YRTDevice dev, YRTHandle framebuffer, int32_t* iterations, float* error, size_t numTiles) {
  DEV_GUARD(dev, -1)
  auto F = dev->d->get<FrameBufferObj>(framebuffer, "framebuffer");
  if (!F) throw std::runtime_error("yrtGetAdaptiveTiles: null handle");
  const size_t n = std::min(numTiles, F->tileIterations.size());
  if (iterations && n) memcpy(iterations, F->tileIterations.data(), n * sizeof(int32_t));
  if (error && n) memcpy(error, F->tileError.data(), n * sizeof(float));
  return (int)F->tileIterations.size();
  DEV_END(-1)
}

int yrtDebugTileError(const float* accu4, const float* half4, int width, int height, float* errorPerTile) {
  if (!accu4 || !half4 || !errorPerTile || width < 1 || height < 1) return -1;
  const int tilesX = (width + 15) / 16, tilesY = (height + 15) / 16;
  for (int ty = 0; ty < tilesY; ++ty)
    for (int tx = 0; tx < tilesX; ++tx)
      errorPerTile[(size_t)ty * tilesX + tx] = yrt_tile_error(accu4, half4, width, height, tx, ty);
  return 0;
}

}  // extern "C"
