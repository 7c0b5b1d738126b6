// pathtrace.hip — wavefront path tracer for gfx950 (MI355X).
//
// The reference's per-pixel integrator (integrators/pathtraceintegrator.cpp:50-217 called
// from renderers/integratorrenderer.cpp:118-185) becomes, per batch of pixels x spp paths:
//
//   k_raygen -> for depth d: k_trace_closest -> k_shade -> k_trace_any -> k_shadow_resolve
//            -> k_resolve_pixels
//
// Queues are compacted with one wave-wide ballot/prefix + one atomic per wave.  Per-path
// radiance is accumulated in the same order as the reference's sequential loop (env or
// emission first, then the direct-light terms in light order), and the pixel sum over
// samples runs s = 0..spp-1, so results do not depend on queue order.
//
// One translation unit: the kernels live in the headers included below, one stage per file;
// this file holds their host launchers.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <set>

#include "yrt_kernels.h"
#include "yrt_wave.h"
#include "yrt_camera.h"
#include "k_raygen.h"
#include "k_trace.h"
#include "yrt_surface.h"
#include "k_shade.h"
#include "k_firsthit.h"
#include "k_denoise.h"
#include "k_tiles.h"
#include "k_checks.h"
#include "k_sample_dirs.h"
#include "k_refit.h"
#include "k_adaptive.h"

namespace yrt {

// ---------------------------------------------------------------- launchers

static inline int grid_for(long long n, int block, int maxBlocks) {
  long long g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > maxBlocks) g = maxBlocks;
  return (int)g;
}

void launch_sample_dirs(const float* pairs, int numRecords, int numSlots, float4* out, hipStream_t s) {
  const int n = numSlots * numRecords;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sample_dirs, dim3((n + 255) / 256), dim3(256), 0, s, pairs, numRecords, numSlots, out);
}

void launch_pixel_sets(const FrameView& fv, uint8_t* pixelSets, int width, int height, int sets, hipStream_t s) {
  const int tiles = ((width + 15) / 16) * ((height + 15) / 16);
  hipLaunchKernelGGL(k_pixel_sets, dim3((tiles + 63) / 64), dim3(64), 0, s, fv.rp, pixelSets);
}

void launch_raygen(const FrameView& fv, const PathBuffers& pb, const BatchInfo& bi, hipStream_t s) {
  // spp is read on device; the host passes the path count through capacity sizing.
#ifndef YRT_RAYGEN_GRID
#define YRT_RAYGEN_GRID 16384
#endif
  hipLaunchKernelGGL(k_raygen, dim3(grid_for(pb.capacity, YRT_BLOCK, YRT_RAYGEN_GRID)), dim3(YRT_BLOCK), 0, s, fv, pb, bi);
}

// closest hit: the kernel's int output (occOut, the any-hit occlusion flags) is unused
void launch_trace_closest(const SceneView& sv, const float4* org, const float4* dir, const unsigned* counts,
                          int numSegs, int segCap, float4* hit, hipStream_t s, const float* time) {
  const dim3 grid(grid_for((long long)numSegs * segCap, YRT_TRACE_BLOCK, YRT_TRACE_GRID));
  if (time)
    hipLaunchKernelGGL((k_trace<false, true>), grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, org, dir, counts, numSegs, segCap,
                       hit, (int*)nullptr, sv.traceSpill, ShadowFuse{}, time, PrimaryRays{});
  else
    hipLaunchKernelGGL((k_trace<false, false>), grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, org, dir, counts, numSegs,
                       segCap, hit, (int*)nullptr, sv.traceSpill, ShadowFuse{}, (const float*)nullptr, PrimaryRays{});
}

void launch_trace_primary(const SceneView& sv, const PrimaryRays& pr, float4* hit, hipStream_t s) {
  const dim3 grid(grid_for(pr.numPaths, YRT_TRACE_BLOCK, YRT_TRACE_GRID));
  hipLaunchKernelGGL((k_trace<false, false, 1>), grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, (const float4*)nullptr,
                     (const float4*)nullptr, (const unsigned*)nullptr, 0, 0, hit, (int*)nullptr, sv.traceSpill,
                     ShadowFuse{}, (const float*)nullptr, pr);
}

void launch_trace_any(const SceneView& sv, const float4* org, const float4* dir, const unsigned* counts, int numSegs,
                      int segCap, int* occluded, hipStream_t s, const ShadowFuse* fuse, const float* time) {
  const dim3 grid(grid_for((long long)numSegs * segCap, YRT_TRACE_BLOCK, YRT_TRACE_GRID));
  const ShadowFuse sf = fuse ? *fuse : ShadowFuse{};
  if (time)
    hipLaunchKernelGGL((k_trace<true, true>), grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, org, dir, counts, numSegs,
                       segCap, (float4*)nullptr, occluded, sv.traceSpill, sf, time, PrimaryRays{});
  else
    hipLaunchKernelGGL((k_trace<true, false>), grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, org, dir, counts, numSegs,
                       segCap, (float4*)nullptr, occluded, sv.traceSpill, sf, (const float*)nullptr, PrimaryRays{});
}

// Instantiated material sets (bitmask of MAT_x): the launcher picks the smallest superset of
// the scene's material and light types; YRT_SV_ALL is the generic fallback.
// Bits 16.. select the light types (light_bit); the first four cover the reference's scenes
// (dome / quad / HDRI lights).
#define YRT_SV_UBER (mat_bit(MAT_UBER) | YRT_BASIC_LIGHTS)                                   // Collada (Sponza)
#define YRT_SV_OBJ (mat_bit(MAT_OBJ) | YRT_BASIC_LIGHTS)                                     // OBJ scenes
#define YRT_SV_SPHERES (mat_bit(MAT_MATTE) | mat_bit(MAT_METALLIC_PAINT) | YRT_BASIC_LIGHTS)  // cornell spheres
#define YRT_SV_STEREO \
  (mat_bit(MAT_UBER) | mat_bit(MAT_MATTE_TEXTURED) | mat_bit(MAT_METALLIC_PAINT) | YRT_BASIC_LIGHTS)  // test_stereo
// the material types DAELoader emits (Matte default, Uber, ThinDielectric for A_ONE
// transparency; devices/device/loaders/ColladaLoader.cpp:102,210-294): every StartRT .dae job
#define YRT_SV_COLLADA \
  (mat_bit(MAT_MATTE) | mat_bit(MAT_UBER) | mat_bit(MAT_THIN_DIELECTRIC) | YRT_BASIC_LIGHTS)
#define YRT_SV_ALL (YRT_ALL_MATS | YRT_ALL_LIGHTS)
static const unsigned kShadeVariants[] = {YRT_SV_UBER,   YRT_SV_OBJ,     YRT_SV_SPHERES,
                                          YRT_SV_STEREO, YRT_SV_COLLADA, YRT_SV_ALL};

template <unsigned MM>
static void launch_shade_t(const SceneView& sv, const FrameView& fv, const PathBuffers& pb, const BatchInfo& bi,
                           int depth, hipStream_t s) {
#ifndef YRT_SHADE_GRID
#define YRT_SHADE_GRID 16384  // blocks of YRT_BLOCK; swept 2048..32768 (x 256 and 64 lanes)
#endif
  hipLaunchKernelGGL(k_shade<MM>, dim3(grid_for(pb.capacity, YRT_BLOCK, YRT_SHADE_GRID)),
                     dim3(YRT_BLOCK), 0, s, sv, fv, pb,
                     bi, depth);
}

void launch_shade(const SceneView& sv, const FrameView& fv, const PathBuffers& pb, const BatchInfo& bi, int depth,
                  unsigned materialMask, hipStream_t s) {
  unsigned pick = YRT_SV_ALL;
  for (unsigned v : kShadeVariants)
    if ((materialMask & ~v) == 0) {
      pick = v;
      break;
    }
  switch (pick) {
    case YRT_SV_UBER: launch_shade_t<YRT_SV_UBER>(sv, fv, pb, bi, depth, s); break;
    case YRT_SV_OBJ: launch_shade_t<YRT_SV_OBJ>(sv, fv, pb, bi, depth, s); break;
    case YRT_SV_SPHERES: launch_shade_t<YRT_SV_SPHERES>(sv, fv, pb, bi, depth, s); break;
    case YRT_SV_STEREO: launch_shade_t<YRT_SV_STEREO>(sv, fv, pb, bi, depth, s); break;
    case YRT_SV_COLLADA: launch_shade_t<YRT_SV_COLLADA>(sv, fv, pb, bi, depth, s); break;
    default: {
      // the generic kernel (every material and light type) holds ~218 VGPRs, 2 waves/SIMD:
      // say so once per material set, so a scene outside the specialized sets is not slow
      // without a trace
      static std::mutex mu;
      static std::set<unsigned> warned;
      {
        std::lock_guard<std::mutex> lk(mu);
        if (warned.insert(materialMask).second)
          fprintf(stderr,
                  "yrt: material/light set 0x%x has no specialized k_shade; using the generic kernel "
                  "(2 waves/SIMD, slower shading)\n",
                  materialMask);
      }
      launch_shade_t<YRT_SV_ALL>(sv, fv, pb, bi, depth, s);
      break;
    }
  }
}

void launch_shadow_resolve(const PathBuffers& pb, int depth, int numLights, hipStream_t s) {
  hipLaunchKernelGGL(k_shadow_resolve, dim3(grid_for(pb.capacity, YRT_BLOCK, 8192)), dim3(YRT_BLOCK),
                     0, s, pb, depth,
                     numLights);
}

void launch_resolve_pixels(const FrameView& fv, const PathBuffers& pb, const BatchInfo& bi, float* fbFloat,
                           uint8_t* fbRGB8, int rgb8Stride, float4* accu, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(k_resolve_pixels, dim3(grid_for(bi.numPixels, YRT_BLOCK, 8192)), dim3(YRT_BLOCK), 0, s, fv, pb, bi,
                     fbFloat, fbRGB8, rgb8Stride, accu, accumulate);
}

void launch_tile_error(const float4* accu, const float4* half, int width, int height, int numTilesX, const int* list,
                       int count, float threshold, int iterations, float* tileError, int* tileIterations, int* stopped,
                       hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_tile_error, dim3(count), dim3(YRT_ADAPTIVE_BLOCK), 0, s, accu, half, width, height, numTilesX,
                     list, count, threshold, iterations, tileError, tileIterations, stopped);
}

void launch_tile_compact(const int* listIn, const int* stopped, int count, int* listOut, int* countOut, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_tile_compact, dim3((count + YRT_ADAPTIVE_BLOCK - 1) / YRT_ADAPTIVE_BLOCK),
                     dim3(YRT_ADAPTIVE_BLOCK), 0, s, listIn, stopped, count, listOut, countOut);
}

void launch_pack_tiles(const float* fbFloat, const uint8_t* fbRGB8, const SlabLayout& L, int numTiles, void* slab,
                       hipStream_t s) {
  const int n = numTiles * 256;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pack_tiles, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, fbFloat, fbRGB8, L, n, slab);
}

void launch_unpack_tiles(const void* slab, float* fbFloat, uint8_t* fbRGB8, const SlabLayout& L, int numTiles,
                         hipStream_t s) {
  const int n = numTiles * 256;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_unpack_tiles, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, slab, fbFloat, fbRGB8, L, n);
}

int check_math_table(int fn, const uint16_t* table2048, unsigned long long* host2) {
  if (fn != 1 && fn != 2) return -1;
  unsigned long long* d = nullptr;
  uint16_t* t = nullptr;
  if (hipMalloc(&d, 16) != hipSuccess) return -1;
  if (hipMalloc(&t, 4096) != hipSuccess) { (void)hipFree(d); return -1; }
  const unsigned long long init[2] = {0ull, ~0ull};
  int rc = 0;
  if (hipMemcpy(d, init, 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(t, table2048, 4096, hipMemcpyHostToDevice) != hipSuccess)
    rc = -1;
  if (!rc) {
    hipLaunchKernelGGL(k_check_math_table, dim3(8192), dim3(256), 0, 0, fn, t, d);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host2, d, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
  }
  (void)hipFree(t);
  (void)hipFree(d);
  return rc;
}

int check_shade(int mode, int n, const float* rows, const GpuMaterial* mats, int numMats, const GpuCamera* cam,
                const GpuLight* light, float* out) {
  if (mode < 0 || mode > 3 || n < 1 || !rows || !out) return -1;
  if ((mode == 2 && !cam) || (mode == 3 && !light)) return -1;
  // every index the kernel follows is checked here: the component count and kinds, and the
  // material record of a conductor component
  for (int i = 0; i < n && mode < 2; ++i) {
    const float* r = rows + (size_t)i * YRT_SHADE_ROW;
    int nc;
    memcpy(&nc, r + 21, 4);
    if (nc < 1 || nc > YRT_MAX_COMPS) return -1;
    for (int k = 0; k < nc; ++k) {
      int kind, id;
      memcpy(&kind, r + 24 + 8 * k, 4);
      memcpy(&id, r + 24 + 8 * k + 6, 4);
      if (kind < 0 || kind > C_DIEL_LAYER_GLITTER) return -1;
      if ((kind == C_CONDUCTOR || kind == C_MICRO_COND || kind == C_MICRO_ANISO) && (!mats || id < 0 || id >= numMats))
        return -1;
    }
  }
  float *dRows = nullptr, *dOut = nullptr;
  GpuMaterial* dMats = nullptr;
  GpuCamera* dCam = nullptr;
  GpuLight* dLight = nullptr;
  const size_t rowBytes = (size_t)n * YRT_SHADE_ROW * sizeof(float), outBytes = (size_t)n * YRT_SHADE_OUT * sizeof(float);
  int rc = 0;
  if (hipMalloc(&dRows, rowBytes) != hipSuccess || hipMalloc(&dOut, outBytes) != hipSuccess ||
      hipMalloc(&dMats, sizeof(GpuMaterial) * (size_t)(numMats > 0 ? numMats : 1)) != hipSuccess ||
      hipMalloc(&dCam, sizeof(GpuCamera)) != hipSuccess || hipMalloc(&dLight, sizeof(GpuLight)) != hipSuccess)
    rc = -1;
  if (!rc && hipMemcpy(dRows, rows, rowBytes, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
  if (!rc && mats && numMats > 0 &&
      hipMemcpy(dMats, mats, sizeof(GpuMaterial) * (size_t)numMats, hipMemcpyHostToDevice) != hipSuccess)
    rc = -1;
  if (!rc && cam && hipMemcpy(dCam, cam, sizeof(GpuCamera), hipMemcpyHostToDevice) != hipSuccess) rc = -1;
  if (!rc && light && hipMemcpy(dLight, light, sizeof(GpuLight), hipMemcpyHostToDevice) != hipSuccess) rc = -1;
  if (!rc) {
    hipLaunchKernelGGL(k_check_shade, dim3((n + 63) / 64), dim3(64), 0, 0, mode, n, dRows, dMats, dCam, dLight, dOut);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = -1;
  }
  (void)hipFree(dLight);
  (void)hipFree(dCam);
  (void)hipFree(dMats);
  (void)hipFree(dOut);
  (void)hipFree(dRows);
  return rc;
}

// the names yrtDebugMaterial's caller gives kShadeVariants' sets, in their order
static const char* const kShadeVariantNames[] = {"uber", "obj", "spheres", "stereo", "collada", "all"};

int shade_variant_index(const char* name) {
  for (int i = 0; i < (int)(sizeof(kShadeVariants) / sizeof(kShadeVariants[0])); ++i)
    if (name && !strcmp(name, kShadeVariantNames[i])) return i;
  return -1;
}

template <unsigned MM>
static void launch_check_material_t(const SceneView& sv, int geom, int medium, int n, const float* rows, float* out) {
  hipLaunchKernelGGL(k_check_material<MM>, dim3((n + 63) / 64), dim3(64), 0, 0, sv, geom, medium, n, rows, out);
}

int check_material(const SceneView& sv, int mode, int variant, int matType, int geom, int medium, int n,
                   const float* rows, float* out) {
  if ((mode != 0 && mode != 1) || n < 1 || !rows || !out || geom < 0) return -1;
  if (variant < 0 || variant >= (int)(sizeof(kShadeVariants) / sizeof(kShadeVariants[0]))) return -1;
  // a material outside the named set is not launched: its case is not compiled into that instantiation
  if (mode == 0 && (matType < 1 || matType > 31 || !(kShadeVariants[variant] & mat_bit(matType)))) return -2;
  const size_t rowBytes = (size_t)n * (mode == 0 ? YRT_MAT_ROW : 2) * sizeof(float);
  const size_t outBytes = (size_t)n * (mode == 0 ? YRT_MAT_OUT : YRT_TEX_OUT) * sizeof(float);
  float *dRows = nullptr, *dOut = nullptr;
  int rc = 0;
  if (hipMalloc(&dRows, rowBytes) != hipSuccess || hipMalloc(&dOut, outBytes) != hipSuccess) rc = -1;
  if (!rc && hipMemcpy(dRows, rows, rowBytes, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
  if (!rc) {
    if (mode == 1) {
      hipLaunchKernelGGL(k_check_textures, dim3((n + 63) / 64), dim3(64), 0, 0, sv, geom, n, dRows, dOut);
    } else {
      switch (kShadeVariants[variant]) {
        case YRT_SV_UBER: launch_check_material_t<YRT_SV_UBER>(sv, geom, medium, n, dRows, dOut); break;
        case YRT_SV_OBJ: launch_check_material_t<YRT_SV_OBJ>(sv, geom, medium, n, dRows, dOut); break;
        case YRT_SV_SPHERES: launch_check_material_t<YRT_SV_SPHERES>(sv, geom, medium, n, dRows, dOut); break;
        case YRT_SV_STEREO: launch_check_material_t<YRT_SV_STEREO>(sv, geom, medium, n, dRows, dOut); break;
        case YRT_SV_COLLADA: launch_check_material_t<YRT_SV_COLLADA>(sv, geom, medium, n, dRows, dOut); break;
        default: launch_check_material_t<YRT_SV_ALL>(sv, geom, medium, n, dRows, dOut); break;
      }
    }
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = -1;
  }
  (void)hipFree(dOut);
  (void)hipFree(dRows);
  return rc;
}

int check_dir_terms(int mode, int n, const float* u, const float* v, float* out4) {
  if ((mode != 0 && mode != 1) || n < 1 || !u || !v || !out4) return -1;
  float* dIn = nullptr;  // the u row, then the v row
  float4* dOut = nullptr;
  const size_t rowBytes = (size_t)n * sizeof(float);
  int rc = 0;
  if (hipMalloc(&dIn, 2 * rowBytes) != hipSuccess || hipMalloc(&dOut, (size_t)n * sizeof(float4)) != hipSuccess) rc = -1;
  if (!rc && (hipMemcpy(dIn, u, rowBytes, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dIn + n, v, rowBytes, hipMemcpyHostToDevice) != hipSuccess))
    rc = -1;
  if (!rc) {
    if (mode == 0)
      hipLaunchKernelGGL(k_check_dir_terms, dim3((n + 63) / 64), dim3(64), 0, 0, dIn, dIn + n, n, dOut);
    else
      launch_sample_dirs(dIn, n, 1, dOut, 0);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out4, dOut, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
      rc = -1;
  }
  (void)hipFree(dOut);
  (void)hipFree(dIn);
  return rc;
}

int check_math(int fn, unsigned long long* host2) {
  if (fn == 3 || fn == 4) {
    // host2[0] = n, host2[1 .. n] = the inputs' bits, replaced by the results' bits
    const unsigned long long n = host2[0];
    if (n < 1 || n > kCheckMathMaxValues) return -1;
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, n * 8) != hipSuccess) return -1;
    int rc = hipMemcpy(d, host2 + 1, n * 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (!rc) {
      hipLaunchKernelGGL(k_check_math_values, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (int)n, d);
      if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host2 + 1, d, n * 8, hipMemcpyDeviceToHost) != hipSuccess)
        rc = -1;
    }
    (void)hipFree(d);
    return rc;
  }
  if (fn != 0) return -1;
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, 16) != hipSuccess) return -1;
  const unsigned long long init[2] = {0ull, ~0ull};
  int rc = 0;
  if (hipMemcpy(d, init, 16, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
  if (!rc) {
    hipLaunchKernelGGL(k_check_math, dim3(8192), dim3(256), 0, 0, fn, d);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host2, d, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
  }
  (void)hipFree(d);
  return rc;
}

int debug_pixel_capture(int pixelId, int frame, float4* out, int capacity) {
  const int v[3] = {pixelId, frame, out ? capacity : 0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_dbgPixel), v, sizeof(v)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_dbgOut), &out, sizeof(out)) != hipSuccess) return -1;
  return 0;
}

int trace_profile(unsigned long long* out8, int reset) {
#if defined(YRT_PROFILE) || defined(YRT_SHADE_PROF)
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_traceProfile), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_traceProfile), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
#else
  (void)out8;
  (void)reset;
  return -1;
#endif
}

void launch_pick(const SceneView& sv, const GpuCamera* cam, float x, float y, float4* out, hipStream_t s) {
  hipLaunchKernelGGL(k_pick, dim3(1), dim3(YRT_TRACE_BLOCK), 0, s, sv, cam, x, y, out);
}

void launch_guides(const SceneView& sv, const GpuCamera* cams, int faces, int width, int height, float4* pos4,
                   float4* nrm4, float4* albedo4, hipStream_t s) {
  const long long n = (long long)width * height;
  if (n <= 0 || faces <= 0) return;
  const dim3 grid((unsigned)((n + YRT_TRACE_BLOCK - 1) / YRT_TRACE_BLOCK), (unsigned)faces);
  hipLaunchKernelGGL(albedo4 ? k_guides<true> : k_guides<false>, grid, dim3(YRT_TRACE_BLOCK), 0, s, sv, cams, width,
                     height, pos4, nrm4, albedo4);
}

void launch_atrous_load(const FrameIO* faceIo, int faces, int width, int height, float4* dst, const Demodulation& dm,
                        hipStream_t s) {
  const long long n = (long long)width * height;
  if (n <= 0 || faces <= 0) return;
  const dim3 grid((unsigned)((n + YRT_BLOCK - 1) / YRT_BLOCK), (unsigned)faces);
  hipLaunchKernelGGL(dm.mod4 ? k_atrous_load<true> : k_atrous_load<false>, grid, dim3(YRT_BLOCK), 0, s, faceIo, width,
                     height, dst, dm.albedo4, dm.albedoFloor, dm.albedoPower, dm.mod4);
}

void launch_atrous(const AtrousParams& ap, int faces, bool wrap, const float4* pos4, const float4* nrm4,
                   const float4* src, float4* dst, const FrameIO* faceOut, const float4* mod4, hipStream_t s) {
  const long long n = (long long)ap.width * ap.height;
  if (n <= 0 || faces <= 0) return;
  const dim3 grid((unsigned)((n + YRT_BLOCK - 1) / YRT_BLOCK), (unsigned)faces);
  const auto kernel = mod4 ? (wrap ? k_atrous<true, true> : k_atrous<true, false>)
                           : (wrap ? k_atrous<false, true> : k_atrous<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(YRT_BLOCK), 0, s, ap, pos4, nrm4, src, dst, mod4, faceOut);
}

void launch_frame_variance(const float4* accu, const float4* half, int width, int height, float gamma, float rcpGamma,
                           int vignetting, float4* var4, hipStream_t s) {
  const long long n = (long long)width * height;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_frame_variance, dim3((unsigned)((n + YRT_BLOCK - 1) / YRT_BLOCK)), dim3(YRT_BLOCK), 0, s, accu,
                     half, width, height, gamma, rcpGamma, vignetting, var4);
}

void launch_atrous_load_var(const FrameIO* faceIo, int faces, int width, int height, float4* dst,
                            const Demodulation& dm, const float4* var4, const float4* pos4, hipStream_t s) {
  const long long n = (long long)width * height;
  if (n <= 0 || faces <= 0) return;
  const dim3 grid((unsigned)((n + YRT_BLOCK - 1) / YRT_BLOCK), (unsigned)faces);
  hipLaunchKernelGGL(dm.mod4 ? k_atrous_load_var<true> : k_atrous_load_var<false>, grid, dim3(YRT_BLOCK), 0, s, faceIo,
                     width, height, dst, dm.albedo4, dm.albedoFloor, dm.albedoPower, dm.mod4, var4, pos4);
}

void launch_atrous_var(const AtrousParams& ap, int faces, bool wrap, const float4* pos4, const float4* nrm4,
                       const float4* src, float4* dst, const FrameIO* faceOut, const float4* mod4, float sigmaVariance2,
                       float varianceFloor, hipStream_t s) {
  const long long n = (long long)ap.width * ap.height;
  if (n <= 0 || faces <= 0) return;
  const dim3 grid((unsigned)((n + YRT_BLOCK - 1) / YRT_BLOCK), (unsigned)faces);
  const auto kernel = mod4 ? (wrap ? k_atrous_var<true, true> : k_atrous_var<true, false>)
                           : (wrap ? k_atrous_var<false, true> : k_atrous_var<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(YRT_BLOCK), 0, s, ap, pos4, nrm4, src, dst, mod4, faceOut, sigmaVariance2,
                     varianceFloor);
}

void launch_debug_render(const SceneView& sv, const FrameView& fv, int maxDepth, int spp, int numTiles, float* fbFloat,
                         uint8_t* fbRGB8, int rgb8Stride, hipStream_t s) {
  hipLaunchKernelGGL(k_debug, dim3((numTiles + 63) / 64), dim3(64), 0, s, sv, fv, maxDepth, spp, fbFloat, fbRGB8,
                     rgb8Stride);
}

#ifdef YRT_PATH_DEBUG
extern "C" int yrt_debug_path(int pixelId, int sample, float* out) {
  if (!out) {
    const int v[2] = {pixelId, sample};
    static const float z[32 * 32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dbgTrace), z, sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_dbgPath), v, sizeof(v)) == hipSuccess ? 0 : -1;
  }
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbgTrace), sizeof(g_dbgTrace)) == hipSuccess ? 0 : -1;
}
#endif

void launch_quantize_nodes(const GpuNode* nodes, GpuQNode* qnodes, int count, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_quantize_nodes, dim3((count + YRT_BLOCK - 1) / YRT_BLOCK), dim3(YRT_BLOCK), 0, s, nodes, qnodes,
                     count);
}

void launch_refit_tris(GpuTri* tris, GpuTriShade* triShade, const int4* indices, const float4* positions,
                       const float4* normals, const int* leafStart, const int* leafSlots, int firstTri, int numTris,
                       hipStream_t s) {
  if (numTris <= 0) return;
  hipLaunchKernelGGL(k_refit_tris, dim3((numTris + YRT_BLOCK - 1) / YRT_BLOCK), dim3(YRT_BLOCK), 0, s, tris, triShade,
                     indices, positions, normals, leafStart, leafSlots, firstTri, numTris);
}

void launch_refit_nodes(GpuNode* nodes, const GpuTri* tris, const int4* indices, const float4* positions,
                        const int* levelNodes, int count, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_refit_nodes, dim3((count + YRT_BLOCK - 1) / YRT_BLOCK), dim3(YRT_BLOCK), 0, s, nodes, tris,
                     indices, positions, levelNodes, count);
}

}  // namespace yrt
