/* yrt_device.h — C ABI of the MI355X path-tracing device plugin (libdevice_singleray_mi355x.so).
 *
 * This is the reference's device plugin boundary made C-callable. Each entry point
 * replaces one virtual method of embree::Device (devices/device/device.h:51-330) with the
 * same arguments and semantics; the plugin factory replaces
 * `extern "C" Device* create(const char* parms, size_t numThreads, int threadsPriority,
 * const char* rtcore_cfg)` (devices/device_singleray/api/singleray_device.cpp:105-107,
 * resolved by devices/device/device.cpp:24-35).
 *
 * Conventions
 *   - Handles are opaque pointers to ref-counted objects starting at refcount 1
 *     (device_singleray/api/handle.h:26-31). yrtIncRef/yrtDecRef mirror rtIncRef/rtDecRef.
 *   - rtSet* values are buffered; yrtCommit (re)constructs the object (api/handle.h:99-103).
 *   - The reference throws std::runtime_error; here every call returns 0 on success and a
 *     negative code on failure, with the message in yrtGetLastError(device). No exception
 *     crosses the ABI.
 *   - Every call on one device is serialized by a device mutex (singleray_device.cpp:97).
 *   - yrtRenderFrame is synchronous (integratorrenderer.cpp:90-93); yrtMapFrameBuffer
 *     returns the host pixel pointer (singleray_device.cpp:439-447). The frame stays in HBM
 *     until the first yrtMapFrameBuffer of that buffer copies it to the host pixels (every
 *     read of the pixels goes through the map, as in the reference); framebuffers created
 *     over user pointers (yrtNewFrameBuffer ptrs) receive the pixels at the end of the render.
 */
#ifndef YRT_DEVICE_H
#define YRT_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YRT_API __attribute__((visibility("default")))

typedef struct YRTDevice_* YRTDevice;
typedef void* YRTHandle;

/* ---- device lifetime (Device::rtCreateDevice / create) ------------------------------ */
/* parms: "" or "device=N" to pick a HIP device; "host" creates a host-only device (loaders,
 * scene commit, BVH build, yrtExportFrame/BVH; rendering and ray queries fail) used by the
 * CPU test suite. numThreads / threadsPriority are accepted
 * for signature parity (they size the CPU TaskScheduler in the reference and are unused
 * on the GPU). */
/* parms: "" or "device=<k>": one HIP device; "devices=<a,b,...>" / "devices=all": the frame's
 * 16x16 tiles are dealt round-robin over several HIP devices, one host
 * thread each, and gathered on the first (RCCL over xGMI between distinct GPUs; an id may
 * repeat for logical shards of one GPU); "host": no GPU (loaders, BVH, frame export). */
YRT_API YRTDevice yrtNewDevice(const char* parms, size_t numThreads, int threadsPriority, const char* rtcore_cfg);
YRT_API void yrtDeleteDevice(YRTDevice dev);
YRT_API const char* yrtGetLastError(YRTDevice dev);

/* ---- object creation (device.h:126-214) ---------------------------------------------- */
YRT_API YRTHandle yrtNewCamera(YRTDevice dev, const char* type);        /* "pinhole", "stereo" */
YRT_API YRTHandle yrtNewData(YRTDevice dev, const char* type, size_t bytes, const void* data);
/* rtNewDataFromFile (device.h:144, singleray_device.cpp:204-222): "immutable" only. */
YRT_API YRTHandle yrtNewDataFromFile(YRTDevice dev, const char* type, const char* file, size_t offset, size_t bytes);
YRT_API YRTHandle yrtNewImage(YRTDevice dev, const char* type, size_t width, size_t height, const void* data);
                                                                       /* "RGB8","RGBA8","RGB_FLOAT32","RGBA_FLOAT32" */
YRT_API YRTHandle yrtNewImageFromFile(YRTDevice dev, const char* file); /* .ppm/.png/.jpg */
YRT_API YRTHandle yrtNewTexture(YRTDevice dev, const char* type);       /* "bilinear","nearest","image" */
YRT_API YRTHandle yrtNewMaterial(YRTDevice dev, const char* type);
YRT_API YRTHandle yrtNewShape(YRTDevice dev, const char* type);         /* "trianglemesh","sphere","triangle" */
YRT_API YRTHandle yrtNewLight(YRTDevice dev, const char* type);         /* "ambientlight","trianglelight","hdrilight" */
YRT_API YRTHandle yrtNewShapePrimitive(YRTDevice dev, YRTHandle shape, YRTHandle material, const float* transform12,
                                       int faceCamera);
YRT_API YRTHandle yrtNewLightPrimitive(YRTDevice dev, YRTHandle light, YRTHandle material, const float* transform12);
/* rtTransformPrimitive (device.h:197): new primitive with transform * prim.transform. */
YRT_API YRTHandle yrtTransformPrimitive(YRTDevice dev, YRTHandle prim, const float* transform12);
YRT_API YRTHandle yrtNewScene(YRTDevice dev, const char* type);
YRT_API int yrtSetPrimitive(YRTDevice dev, YRTHandle scene, size_t slot, YRTHandle prim);
/* rtUpdatePrimitive (device.h:207, singleray_device.cpp:354-398): re-aims a faceCamera
 * primitive at camPos (floor-projected) with up camUp; no-op for other primitives. The scene
 * must be re-committed afterwards, as renderer.cpp:550-559 does per cube face. */
YRT_API int yrtUpdatePrimitive(YRTDevice dev, YRTHandle scene, size_t slot, YRTHandle prim, const float* camPos3,
                               const float* camUp3);
YRT_API YRTHandle yrtNewToneMapper(YRTDevice dev, const char* type);    /* "default" */
YRT_API YRTHandle yrtNewRenderer(YRTDevice dev, const char* type);      /* "pathtracer", "debug" */
YRT_API YRTHandle yrtNewFrameBuffer(YRTDevice dev, const char* type, size_t width, size_t height, size_t buffers,
                                    void** ptrs);

/* ---- reference counting / properties (device.h:237-312) ----------------------------- */
YRT_API int yrtIncRef(YRTDevice dev, YRTHandle h);
YRT_API int yrtDecRef(YRTDevice dev, YRTHandle h);
YRT_API int yrtSetBool1(YRTDevice dev, YRTHandle h, const char* property, int x);
YRT_API int yrtSetBool2(YRTDevice dev, YRTHandle h, const char* property, int x, int y);
YRT_API int yrtSetBool3(YRTDevice dev, YRTHandle h, const char* property, int x, int y, int z);
YRT_API int yrtSetBool4(YRTDevice dev, YRTHandle h, const char* property, int x, int y, int z, int w);
YRT_API int yrtSetInt1(YRTDevice dev, YRTHandle h, const char* property, int x);
YRT_API int yrtSetInt2(YRTDevice dev, YRTHandle h, const char* property, int x, int y);
YRT_API int yrtSetInt3(YRTDevice dev, YRTHandle h, const char* property, int x, int y, int z);
YRT_API int yrtSetInt4(YRTDevice dev, YRTHandle h, const char* property, int x, int y, int z, int w);
YRT_API int yrtSetFloat1(YRTDevice dev, YRTHandle h, const char* property, float x);
YRT_API int yrtSetFloat2(YRTDevice dev, YRTHandle h, const char* property, float x, float y);
YRT_API int yrtSetFloat3(YRTDevice dev, YRTHandle h, const char* property, float x, float y, float z);
YRT_API int yrtSetFloat4(YRTDevice dev, YRTHandle h, const char* property, float x, float y, float z, float w);
YRT_API int yrtGetFloat1(YRTDevice dev, YRTHandle h, const char* property, float* x);
YRT_API int yrtGetFloat3(YRTDevice dev, YRTHandle h, const char* property, float* x, float* y, float* z);
/* rtGetString (device.h:293): copies at most bufSize-1 bytes + NUL; returns the full length. */
YRT_API int yrtGetString(YRTDevice dev, YRTHandle h, const char* property, char* buf, size_t bufSize);
/* rtGetTransform (device.h:303): 12 floats (vx, vy, vz, p); identity when unset. */
YRT_API int yrtGetTransform(YRTDevice dev, YRTHandle h, const char* property, float* transform12);
YRT_API int yrtSetArray(YRTDevice dev, YRTHandle h, const char* property, const char* type, YRTHandle data,
                        size_t size, size_t stride, size_t ofs);
YRT_API int yrtSetString(YRTDevice dev, YRTHandle h, const char* property, const char* str);
YRT_API int yrtSetImage(YRTDevice dev, YRTHandle h, const char* property, YRTHandle image);
YRT_API int yrtSetTexture(YRTDevice dev, YRTHandle h, const char* property, YRTHandle texture);
YRT_API int yrtSetTransform(YRTDevice dev, YRTHandle h, const char* property, const float* transform12);
YRT_API int yrtSetPointer(YRTDevice dev, YRTHandle h, const char* property, void* p);
YRT_API int yrtClear(YRTDevice dev, YRTHandle h);
YRT_API int yrtCommit(YRTDevice dev, YRTHandle h);

/* ---- rendering (device.h:223-234, 322) ----------------------------------------------- */
YRT_API int yrtRenderFrame(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene,
                           YRTHandle tonemapper, YRTHandle framebuffer, int accumulate);
/* Several frames of one scene in one wavefront job: frame k seen through cameras[k] into
 * framebuffers[k] (all the same size and format). With accumulate = 0 the result equals
 * numFrames rtRenderFrame calls with accumulate = 0, bit for bit (the per-tile Random of
 * integratorrenderer.cpp:134 and every per-pixel input depend on the frame's own pixel only),
 * but the frames' 16x16 tiles form one sequence (frame-major) that fills the batches and is
 * dealt over shards and GPUs as a whole, with one gather per job. This is the loop of the
 * stereo-cube drivers over the 12 faces of a view (renderer.cpp:543-737, 742-878) when no
 * primitive changes between the faces. accumulate != 0 is accepted for numFrames == 1 only (a
 * job keeps one sampler iteration and no per-frame accumulation state across calls). For the
 * same reason yrtRenderFrame(..., accumulate = 1) into a framebuffer whose last frame came from a
 * job of several frames fails with an error, until a frame with accumulate = 0 has been rendered
 * into it: the accumulation buffer belongs to the framebuffer, and such a job does not fill it. */
YRT_API int yrtRenderFrames(YRTDevice dev, YRTHandle renderer, const YRTHandle* cameras, int numFrames,
                            YRTHandle scene, YRTHandle tonemapper, const YRTHandle* framebuffers, int accumulate);
YRT_API void* yrtMapFrameBuffer(YRTDevice dev, YRTHandle framebuffer, int bufID);
YRT_API int yrtUnmapFrameBuffer(YRTDevice dev, YRTHandle framebuffer, int bufID);
YRT_API int yrtSwapBuffers(YRTDevice dev, YRTHandle framebuffer);
/* rtPick (device.h:329, singleray_device.cpp:692-708): world position of the closest hit of
 * the camera ray through image-plane point (x, y) in [0,1]^2. Returns 1 hit, 0 miss, <0 error. */
YRT_API int yrtPick(YRTDevice dev, YRTHandle camera, float x, float y, YRTHandle scene, float* px, float* py,
                    float* pz);
/* ---- adaptive sampling: converged 16x16 tiles stop, only the active ones render ----
 * yrtRenderAdaptive renders one frame in progressive iterations of the renderer's committed spp
 * each. It starts like accumulate = 0 (the renderer's iteration is reset, the framebuffer's sums
 * start from this frame); iteration k = 0, 1, ... renders the active tiles with sampler iteration k
 * and adds them into the framebuffer's sums exactly as yrtRenderFrame(..., 1) does, and the even
 * iterations also into a second buffer of the framebuffer, the half buffer. After iteration k,
 * when n = k + 1 is even and n >= minIterations (raised to the next even number, at least 2), the
 * error estimate E_T of every active tile is computed from the two buffers (Dammertz et al. 2010,
 * csrc/common/yrt_tile_error.h; linear radiance, the tone mapper plays no part) and a tile stops
 * iff E_T < threshold (strict; a NaN never stops). A stopped tile is never touched again and keeps
 * the display of its last iteration, so its pixels are, bit for bit, those of n calls of
 * yrtRenderFrame(..., 1). The call ends when no tile is active, at n = maxIterations, or when the
 * renderer's stop flag is set between iterations. threshold <= 0 stops nothing: the call equals
 * maxIterations progressive frames. Afterwards the renderer's iteration is n, and
 * yrtRenderFrame(..., accumulate = 1) into the framebuffer is refused until a frame with
 * accumulate = 0 has been rendered into it.
 * Refused with an error and no launch: the debug renderer, a device with more than one render
 * context (devices=...), an armed tile shard, communicator or hub, armed ray capture,
 * maxIterations < 1 and a non-finite threshold.
 * size = sizeof of the caller's struct, as in YRTDenoiseParams: a shorter params struct is read up
 * to its size, the remaining fields take their defaults (0.05, 2, 64; yrtAdaptiveDefaults), and
 * the stats are written up to the caller's size. out may be NULL. */
typedef struct YRTAdaptiveParams {
  uint32_t size;
  float threshold;
  int minIterations, maxIterations;
} YRTAdaptiveParams;
/* iterations: n. tiles: the frame's tiles; tilesStopped: those the check stopped. samples: the sum
 * of the pixel weights (samples traced inside the image). msTotal: the call; msError: its checks
 * (estimate, compaction and the read of the new tile count), host clock. */
typedef struct YRTAdaptiveStats {
  uint32_t size;
  int32_t iterations;
  int64_t tiles, tilesStopped;
  double samples, msTotal, msError;
} YRTAdaptiveStats;
YRT_API int yrtAdaptiveDefaults(YRTAdaptiveParams* p);
YRT_API int yrtRenderAdaptive(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene,
                              YRTHandle tonemapper, YRTHandle framebuffer, const YRTAdaptiveParams* p,
                              YRTAdaptiveStats* out);
/* The tiles of the framebuffer's last adaptive render in image tile order, row-major: returns
 * their number (0: none yet, -1: error) and fills, for the first numTiles of them, the iterations
 * each ran and its last computed E_T (+inf for a tile no check looked at). Either array may be NULL. */
YRT_API int yrtGetAdaptiveTiles(YRTDevice dev, YRTHandle framebuffer, int32_t* iterations, float* error,
                                size_t numTiles);
/* Host-side: E_T of every tile of a width x height frame from its sums accu4 and half sums half4
 * ([height][width][4] floats: r, g, b, weight), by the header the kernel compiles;
 * errorPerTile holds ceil(width / 16) * ceil(height / 16) floats. -1 on a null pointer or an
 * empty frame. */
YRT_API int yrtDebugTileError(const float* accu4, const float* half4, int width, int height, float* errorPerTile);
/* ---- denoise: first-hit guide buffers and an edge-avoiding a-trous filter ---- */
/* yrtRenderGuides: for pixel (x, y) of a width x height view, rtPick's camera ray through the
 * image-plane point ((x + .5) / width, (y + .5) / height) (time 0 in moving scenes):
 * pos4Host[4 i] = (hit point, t), nrm4Host[4 i] = (shading normal turned towards the viewer, 1),
 * i = y * width + x; a miss gives (0, 0, 0, +inf) and (0, 0, 0, 0). width * height * 4 floats each. */
YRT_API int yrtRenderGuides(YRTDevice dev, YRTHandle camera, YRTHandle scene, int width, int height,
                            float* pos4Host, float* nrm4Host);
/* yrtRenderAlbedo: the first-hit albedo of the same rays, albedo4Host[4 i] = (albedo, 1), a miss
 * (0, 0, 0, 0); width * height * 4 floats. The albedo is the per-channel sum of the reflectances
 * of the diffuse-reflection components the hit's material creates there, textures included
 * (Matte, MatteTextured and Uber x texture x alpha, Obj d Kd map_Kd, the Plastic and MetallicPaint
 * pigment, both Velvet lobes), evaluated in the medium a camera ray starts in; it is (1, 1, 1)
 * where there is no such component (mirror, metal, dielectrics), where the sum is 0 and on a light
 * primitive. The guide normals are postIntersect's: an Obj bump map does not reach them. */
YRT_API int yrtRenderAlbedo(YRTDevice dev, YRTHandle camera, YRTHandle scene, int width, int height,
                            float* albedo4Host);
/* size = sizeof(YRTDenoiseParams) of the caller's build, checked: a shorter struct is read up to
 * its size and the remaining fields take their defaults; below sizeof(size) is an error.
 * iterations: filter passes, step 2^i (0: the call writes nothing). sigmaColor: colour weight
 * exp(-|dc|^2 / (sigmaColor 2^-i)^2), <= 0 turns it off. sigmaNormal: exponent of
 * max(0, n_p . n_q). sigmaPosition: plane-distance weight exp(-|n_p . (x_q - x_p)| /
 * (sigmaPosition t_p)). Defaults: 5, 1, 64, 0.02 (yrtDenoiseDefaults).
 * demodulate != 0: the texture-preserving filter. The frame is divided by the modulation
 * m = max(albedo, albedoFloor) ^ albedoPower per channel (yrtRenderAlbedo's albedo of the pixel),
 * the iterations run on the quotient, colour weight included, and the last one stores the result
 * times m. albedoPower: 1 / gamma of the tone mapper the frame went through, since
 * (a L)^(1/gamma) = a^(1/gamma) L^(1/gamma); the vignette is a per-pixel factor and cancels.
 * albedoFloor keeps the division away from 0. Both must be finite and > 0 and are checked only when
 * demodulate is set; demodulate = 0 (the default, and a struct that ends before it) is the plain
 * filter, bit for bit. Defaults: 0, 1, 1/255.
 * varianceGuided != 0: the variance-guided filter (after SVGF, Schied et al. 2017) for a frame whose
 * framebuffer holds an adaptive render (yrtRenderAdaptive; threshold 0 and maxIterations K are K
 * plain progressive frames). The per-pixel variance of the displayed frame (yrtFrameVariance) is
 * summed over the channels (divided by m^2 per channel when demodulate is set) and filtered along
 * with the colour, v' = sum w^2 v / (sum w)^2, and the colour weight becomes
 * exp(-|dc|^2 / (sigmaVariance^2 vbar + varianceFloor)), vbar the 3x3 Gaussian mean of the
 * variance around the pixel; sigmaColor is not read and nothing tightens with the step.
 * varianceFloor keeps flat regions filtering: (1/255)^2, the square of an 8-bit step. Both must be
 * finite and > 0 and are checked only when varianceGuided is set. The call is refused, and writes
 * nothing, unless every framebuffer's last frame is an adaptive render on this device in which
 * every tile ran at least 2 iterations. varianceGuided = 0 (the default, and a struct that ends
 * before it) is the filter above, bit for bit. Defaults: 0, 3, (1/255)^2. Known limit: on an
 * emitter's edge the honest variance is large and the light bleeds onto coplanar surfaces around it
 * (DESIGN.md §9). */
typedef struct YRTDenoiseParams {
  uint32_t size;
  int iterations;
  float sigmaColor, sigmaNormal, sigmaPosition;
  int demodulate;
  float albedoPower, albedoFloor;
  int varianceGuided;
  float sigmaVariance, varianceFloor;
} YRTDenoiseParams;
/* Fills the fields that fit into p->size (set by the caller) with the library's defaults. */
YRT_API int yrtDenoiseDefaults(YRTDenoiseParams* p);
/* Filters the framebuffer's current buffer in place, guided by the first hits seen through
 * `camera` (the camera the frame was rendered with; a cube face's own). The filter input is the
 * frame as it stands — tone mapped, 8-bit channels as byte / 255 — and the result is stored in
 * the framebuffer's own format; alpha channels, RGB8 row padding and pixels whose camera ray
 * leaves the scene are not written. The frame is filtered where it lives: an RGB8 or
 * RGB_FLOAT32 frame that no rtMapFrameBuffer has read yet is filtered in HBM (and read back
 * filtered by the next map); any other is uploaded from the host pixels, filtered and written
 * back to them. Runs on the device's first GPU, after the gather of a multi-GPU render; under
 * process tile shards (yrtSetTileShard / yrtSetShardComm) call it on the rank that holds the
 * gathered frame (rank 0): it filters whatever the framebuffer holds. p = NULL: defaults. */
YRT_API int yrtDenoiseFrameBuffer(YRTDevice dev, YRTHandle camera, YRTHandle scene, YRTHandle framebuffer,
                                  const YRTDenoiseParams* p);
/* The same filter over a stereo cube as one surface: a tap that leaves a face reads the pixel its
 * direction falls on on the neighbouring face of the same eye (corner taps stay skipped, the eyes
 * never exchange taps), so the cube's edges are filtered like its faces' interiors. numFrames is 6
 * (one eye) or 12; every camera is a committed "stereo" camera, the faces cubeFaceIndex % 6 of each
 * eye (cubeFaceIndex / 6) each present exactly once, in any order, the cameras of one eye equal in
 * everything but cubeFaceIndex; framebuffers[k] holds the frame rendered through cameras[k], all
 * square, of one size (at most 16384) and one format. The cameras must form an ideal cube (what a
 * lookAt perpendicular to `up` gives); otherwise the call fails and writes nothing. p is read as
 * by yrtDenoiseFrameBuffer, and each frame is filtered where it lives, by that call's rules. */
YRT_API int yrtDenoiseCube(YRTDevice dev, const YRTHandle* cameras, int numFrames, YRTHandle scene,
                           const YRTHandle* framebuffers, const YRTDenoiseParams* p);
/* Host-side: the rule that says where a cube filter tap lands (csrc/common/yrt_cube_tap.h). The
 * tap (qx, qy) of face `face` (0..5 within its eye) of W x W faces: returns 1 and (g, x', y') for
 * a tap that lands on a face, 0 for a skipped corner tap, -1 for arguments out of range (W outside
 * 1..16384, a tap farther than 2^17 pixels from the face, a null pointer). */
YRT_API int yrtDebugCubeTap(int W, int face, int qx, int qy, int* g, int* x, int* y);
/* The variance frame of the framebuffer's last adaptive render, the counterpart of yrtRenderGuides
 * for the variance-guided filter: var4Host[4 i] = (v_r, v_g, v_b, 1), i = y * width + x,
 * width * height * 4 floats. With the sums S (weight w) and the half sums H (weight h, the even
 * iterations) of the render and r = w - h: A = H rcp(h), B = max(S - H, 0) rcp(r), both mapped as
 * the render's tone mapper displays them (pow 1 / gamma iff gamma != 1, then the vignette iff set),
 * v_c = (dA_c - dB_c)^2 (h r) rcp(w)^2, the variance of the displayed mean of the two halves; a v_c
 * that is not finite is 0. Refused as the variance-guided filter is: after any other render into
 * the framebuffer, on another device, or when a tile ran fewer than 2 iterations. */
YRT_API int yrtFrameVariance(YRTDevice dev, YRTHandle framebuffer, float* var4Host);
/* The framebuffer's size in pixels (what sizes var4Host); either pointer may be NULL. */
YRT_API int yrtGetFrameBufferSize(YRTDevice dev, YRTHandle framebuffer, int* width, int* height);
/* Host-side: the same estimate by the header the kernel compiles (csrc/common/yrt_pixel_variance.h)
 * from sums accu4 and half sums half4 ([height][width][4] floats: r, g, b, weight) into var4 (the
 * same shape). With gamma 1 and vignetting 0 it equals the device's bit for bit. -1 on a null
 * pointer or an empty frame. */
YRT_API int yrtDebugFrameVariance(const float* accu4, const float* half4, int width, int height, float gamma,
                                  int vignetting, float* var4);
/* With yrtSetKernelTiming on: HIP-event times, in ms, of the kernels of the last guide pass
 * (yrtRenderGuides, yrtRenderAlbedo, or the one inside yrtDenoiseFrameBuffer / yrtDenoiseCube, which renders the
 * albedo in the same kernel when demodulate is set) and of the last filter (its load and
 * iterations and, variance-guided, its variance pass; without the guide pass and any host copy). Either pointer may be NULL. */
YRT_API int yrtGetDenoiseTimes(YRTDevice dev, float* msGuides, float* msFilter);
/* Renderer status callback (device.h:335-347): state 0 Inactive, 1 Rendering, 2 Done. */
typedef void (*YRTStatusCallback)(int state, float progress, void* user);
YRT_API int yrtSetStatusCallback(YRTDevice dev, YRTHandle renderer, YRTStatusCallback cb, void* user);
/* Stop flag polled between wavefront iterations (renderer "stopFlag", integratorrenderer.h:100). */
YRT_API int yrtSetStopFlag(YRTDevice dev, YRTHandle renderer, volatile int* flag);

/* ---- hot-path ray queries: rtcIntersect / rtcOccluded over device-resident streams ---- */
/* org4[i] = (org.xyz, tnear), dir4[i] = (dir.xyz, tfar) ; hit4[i] = (t, u, v, triId bits)
 * occluded[i] = 1/0. All pointers are HIP device pointers; stream may be NULL (default).
 * Replaces rtcIntersect (pathtraceintegrator.cpp:72) and rtcOccluded (:160). */
YRT_API int yrtIntersect(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, uint32_t n,
                         float* hit4, void* stream);
YRT_API int yrtOccluded(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, uint32_t n,
                        int32_t* occluded, void* stream);
/* The same queries with a time per ray (Ray::time): time[i], n floats in device memory. On a scene
 * with moving geometry (a mesh with "motions", a sphere with dPdt) ray i meets every triangle at
 * p + time[i] * m. time[i] lies in [0, 1], the span the BVH's boxes cover; a value outside it or
 * a NaN is outside the contract (the result is unspecified). A scene without moving geometry
 * ignores the times, as a static mesh ignores Ray::time: the array is accepted and not read.
 * time = NULL is the untimed call, and the untimed call on a moving scene is time 0 for every ray. */
YRT_API int yrtIntersectTimed(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4,
                              const float* time, uint32_t n, float* hit4, void* stream);
YRT_API int yrtOccludedTimed(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4,
                             const float* time, uint32_t n, int32_t* occluded, void* stream);
/* Maps a global triangle id (hit4.w) to Embree's (geomID, primID). */
YRT_API int yrtTriangleIds(YRTDevice dev, YRTHandle scene, int32_t tri, int32_t* geomID, int32_t* primID);

/* ---- statistics of the last yrtRenderFrame (integratorrenderer.cpp:96-116) ------------ */
typedef struct YRTRenderStats {
  double raysClosest;     /* rtcIntersect-equivalent queries  */
  double raysShadow;      /* rtcOccluded-equivalent queries   */
  double samples;         /* W*H*spp                          */
  double msTotal;         /* wall time of yrtRenderFrame      */
  double msTraceClosest;  /* summed kernel time (HIP events) when timing enabled */
  double msTraceShadow;
  double msShade;
  double msOther;
  double launchesClosest; /* kernel launches of each kind */
  double launchesShadow;
  double nodeVisits;      /* reserved (0): visit counts come from oracle_count_visits */
  double triVisits;
  double gather;          /* how the frame was gathered: YRT_GATHER_* */
  double msRender;        /* wall time until this process's tiles were rendered (multi-GPU diagnosis) */
  double msGather;        /* wall time of the gather after that (0 without one; includes waiting for peers) */
} YRTRenderStats;
#define YRT_GATHER_NONE 0           /* one device, no gather */
#define YRT_GATHER_D2D 1            /* logical shards of one GPU: device-to-device copy */
#define YRT_GATHER_RCCL_LOCAL 2     /* distinct GPUs of one process: RCCL (ncclCommInitAll) send/recv */
#define YRT_GATHER_PEER_COPY 3      /* distinct GPUs, RCCL unavailable or timed out: hipMemcpyPeerAsync */
#define YRT_GATHER_RCCL_PROCESS 4   /* one process per GPU: RCCL communicator (yrtSetShardComm) */
#define YRT_GATHER_HUB 5            /* several devices of one process: shard hub (yrtSetShardHub) */
YRT_API int yrtGetRenderStats(YRTDevice dev, YRTRenderStats* out);
/* 1 = bracket every kernel with HIP events (adds sync-free event records). */
YRT_API int yrtSetKernelTiming(YRTDevice dev, int enable);
/* Wavefront lanes (HIP streams whose batches overlap) of every render context, 1..4; 0 = the
 * default (3, or YRT_LANES). With one lane no two kernels of a frame overlap, so the kernel
 * timings above are each kernel's own duration (bench.py's roofline uses such a frame). */
YRT_API int yrtSetLanes(YRTDevice dev, int lanes);
/* Scene info: triangles, geometries, BVH nodes, BVH depth, build seconds; numTriRefs = leaf
 * triangle records (>= numTriangles: spatial splits reference a triangle from several leaves). */
typedef struct YRTSceneInfo {
  int64_t numTriangles, numGeometries, numNodes, bvhDepth, numLights;
  double buildSeconds;
  float bboxLo[3], bboxHi[3];
  int64_t numTriRefs;
  int64_t triRecordBytes;  /* bytes per leaf triangle record (48, or 64 with a stored normal) */
  /* bytes per BVH node the closest-hit / any-hit traversal reads: 128 (float planes) or 64
   * (8-bit quantized planes, yulio-raytracer_amd/csrc/common/yrt_qnode.h) */
  int64_t nodeBytesClosest, nodeBytesAny;
} YRTSceneInfo;
YRT_API int yrtGetSceneInfo(YRTDevice dev, YRTHandle scene, YRTSceneInfo* out);
/* The scene builder. yrtSetString(scene, "builder", "morton") before yrtCommit builds the BVH on
 * the GPU: 63-bit Morton keys of the triangles' box centres, a stable radix sort, Karras' radix
 * tree with leaves of up to 8 triangles, collapsed to the same 4-wide nodes (on a "host" device
 * the same steps run in a serial loop and give the same tree). "default" and every other value
 * keep the host's binned-SAH builder; the environment variable YRT_BUILDER=morton makes "default"
 * mean "morton". Hits and frames do not depend on the builder, only the time to build and to
 * traverse. A commit that asks for another builder than the tree's rebuilds; vertex-only commits
 * after a morton build refit as after any other.
 * yrtGetSceneBuildInfo: the BVH step of the scene's last build (not of a refit). size = the bytes
 * of the caller's struct, set by the caller; nothing is written past it.
 *   builder   0 host SAH, 1 morton on the GPU, 2 morton's host loop
 *   fallback  why a morton commit used the host SAH builder after all: 0 it did not, 1 fewer than
 *             2 triangles, 2 a vertex that is not finite, 3 the traversal stack bound would exceed
 *             the kernels' stack, 4 node or reference limits
 *   msBuild   wall time of the BVH step alone, upload and download of a GPU build included
 *             (YRTSceneInfo::buildSeconds is the whole commit)
 *   msKernels HIP-event time of the build kernels with yrtSetKernelTiming on, else 0
 *   sahCost   over every child box of the float nodes: area(child) / area(root) x (1 for an inner
 *             child, the triangle count for a leaf) */
typedef struct YRTSceneBuildInfo {
  uint32_t size;
  int32_t builder, fallback;
  int32_t pad;
  double msBuild, msKernels, sahCost;
} YRTSceneBuildInfo;
YRT_API int yrtGetSceneBuildInfo(YRTDevice dev, YRTHandle scene, YRTSceneBuildInfo* out);
/* Copies the host mirror of the BVH (4-wide nodes: 128 B each, numTriRefs leaf tris: 48 B each). */
YRT_API int yrtExportBVH(YRTDevice dev, YRTHandle scene, void* nodes, size_t nodesBytes, void* tris,
                         size_t trisBytes);
/* The same tree with the any-hit traversal's 64-byte quantized nodes (node i = node i of
 * yrtExportBVH; layout yulio-raytracer_amd/csrc/common/yrt_qnode.h): numNodes * 64 bytes. */
YRT_API int yrtExportQuantizedBVH(YRTDevice dev, YRTHandle scene, void* qnodes, size_t qnodesBytes);
/* Serializes the committed scene graph + renderer + camera as the oracle's input blob
 * (format: oracle/yrt_oracle.h). Returns the byte count; call with buf=NULL to size. */
YRT_API int64_t yrtExportFrame(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene, void* buf,
                               size_t bytes);
/* Frame seed of the shadow-jitter hash (replaces C rand(), pathtraceintegrator.cpp:151). */
YRT_API int yrtSetFrameSeed(YRTDevice dev, uint32_t seed);
/* Paths in flight per wavefront batch (default 64M, ~10 GB of wavefront state); smaller for tests. */
YRT_API int yrtSetBatchCapacity(YRTDevice dev, int64_t paths);
/* Tile sharding across processes: this process renders only the tiles with
 * (tileIndex % count) == index (dealt further over its own HIP devices, see yrtNewDevice);
 * without a communicator (yrtSetShardComm) the other tiles' pixels are left zero. With a
 * communicator, only its own (rank, world) shard is accepted. */
YRT_API int yrtSetTileShard(YRTDevice dev, int index, int count);
/* Multi-GPU, one process per GPU (the reference's device_network image split,
 * devices/device_network/network_device.cpp:255-300, as an RCCL gather over xGMI):
 * yrtShardCommUniqueId fills 128 bytes on rank 0 (ncclGetUniqueId), which the caller
 * broadcasts; every rank then calls yrtSetShardComm with it. Tiles are dealt round-robin
 * (tile % world == rank) and every rtRenderFrame ends with a grouped RCCL send of each rank's
 * tile slab to rank 0, whose framebuffer then holds the whole frame. */
YRT_API int yrtShardCommUniqueId(void* id128);
/* Every rank of a job calls yrtSetShardComm (collective: RCCL ncclCommInitRank). Before each
 * gather the ranks exchange their render status, so a rank whose render throws (or whose
 * render call fails on its arguments) makes every rank's yrtRenderFrame fail instead of
 * leaving rank 0 waiting. Every wait of the gather is bounded (yrtSetGatherTimeout): on expiry
 * the communicator is aborted (ncclCommAbort) and the call fails with the phase that timed
 * out; later gathers on it fail at once. world = 1 drops the communicator. The gathered slabs carry 4 bytes per pixel for RGB8 framebuffers (16 else).
 * Only rank 0's framebuffers receive pixels; the other ranks' host framebuffers are left as
 * they were (their part of the frame is already on rank 0). */
YRT_API int yrtSetShardComm(YRTDevice dev, int rank, int world, const void* id128);
/* The same gather between several devices of one process (threads; they may share a GPU):
 * yrtNewShardHub(world) is the meeting point, and yrtSetShardHub(dev, hub, rank) arms device
 * `rank` (tile shard rank of world) exactly as yrtSetShardComm would; hub = NULL disarms. The
 * slabs move by hipMemcpyPeerAsync (device-to-device on one GPU). This runs the process
 * gather's bookkeeping — status exchange, per-rank tile counts, pack, unpack, the failing-rank
 * path — on one GPU. A device keeps the hub alive; yrtDeleteShardHub drops the caller's. */
typedef struct YRTShardHub_* YRTShardHub;
YRT_API YRTShardHub yrtNewShardHub(int world);
YRT_API void yrtDeleteShardHub(YRTShardHub hub);
YRT_API int yrtSetShardHub(YRTDevice dev, YRTShardHub hub, int rank);
/* Bound, in seconds, of the waits of a gather; default YRT_GATHER_TIMEOUT_S or 300. The slab
 * send/recv wait at most this long; the status exchange, which also waits for the slowest rank's
 * render, this plus ten times the calling rank's render time of the frame. */
YRT_API int yrtSetGatherTimeout(YRTDevice dev, double seconds);
/* Host-memory forms of the hub's two phases (CPU tests of its deadlines and size checks):
 * yrtShardHubStatus returns the min of the ranks' flags (or -1), yrtShardHubSlab sends `bytes`
 * to rank 0 (rank > 0) or receives every peer's recvBytesPerRank bytes into recv in rank
 * order (rank 0). Errors: -1 and yrtShardHubLastError() (per calling thread). */
YRT_API int yrtShardHubStatus(YRTShardHub hub, int rank, int flag, double timeoutS);
YRT_API int yrtShardHubSlab(YRTShardHub hub, int rank, const void* slab, size_t bytes, void* recv,
                            size_t recvBytesPerRank, double timeoutS);
YRT_API const char* yrtShardHubLastError(void);
/* 1 when librccl can be loaded (checked on every rank before the collective comm init). */
YRT_API int yrtRcclAvailable(void);
/* HIP devices (logical shards) this device renders on (yrtNewDevice "devices=..."). */
YRT_API int yrtGetDeviceCount(YRTDevice dev);
/* Scene commits that only move the vertices of some primitives (faceCamera re-orientation by
 * rtUpdatePrimitive, the FPR loop of renderer.cpp:550-559) refit the BVH on the GPU instead of
 * rebuilding it (on by default). yrtGetSceneRefits: refit commits since the last rebuild. */
YRT_API int yrtSetRefitCommits(YRTDevice dev, int on);
YRT_API int yrtGetSceneRefits(YRTDevice dev, YRTHandle scene);
/* Host sampler check: writes the SoA sample table (dims x (sets*spp)) that the frame
 * renderer uploads (sampler/sampler.cpp:46-126 restated); returns sets*spp records. */
/* Ray capture for the roofline's algorithmic bytes: while maxPerDepth > 0,
 * yrtRenderFrame keeps a strided sample (<= maxPerDepth rays) of the closest-hit and shadow
 * query streams of every depth of its first wavefront batch (synchronizes per depth: use on
 * an untimed frame). yrtGetCapturedRays returns the sample size and the stream's full size. */
YRT_API int yrtSetRayCapture(YRTDevice dev, int maxPerDepth);
YRT_API int64_t yrtGetCapturedRays(YRTDevice dev, int shadow, int depth, float* org4, float* dir4, size_t maxRays,
                                   double* totalInBatch);
/* Profiling builds (-DYRT_PROFILE) only: k_trace SIMD-utilization counters since the last
 * reset (outer iterations, lanes with a ray, node-phase iterations, lanes at a node, leaf
 * passes, triangle-loop iterations, useful triangle tests, 0). Returns -1 otherwise. */
YRT_API int yrtDebugTraceProfile(YRTDevice dev, uint64_t* out8, int reset);
/* Arithmetic self-check on the device: fn 0 compares the kernels' correctly rounded fast
 * reciprocal (rcp_rn, common/yrt_math.h) with the IEEE division 1.0f/x for all 2^32 inputs.
 * out2[0] = mismatches, out2[1] = the smallest mismatching input (or UINT64_MAX).
 * fn 3 / 4: the emulated rcpps / rsqrtps (common/yrt_sse_rcp.h) of given inputs: out2[0] = their
 * count n (at most 2^20), out2[1 .. n] = the inputs' bits, replaced by the results' bits. */
YRT_API int yrtDebugCheckMath(YRTDevice dev, int fn, uint64_t* out2);
/* Arithmetic self-check of the emulated SSE estimates the reference's rcp/rsqrt start from
 * (common/yrt_sse_rcp.h; common/math/math.h:38-59): fn 1 rcpps, fn 2 rsqrtps, each against its
 * reconstruction from table2048 (the 12-bit mantissas of tests/golden/sse_rcp_tables.json) for
 * all 2^32 inputs. out2 as yrtDebugCheckMath. */
YRT_API int yrtDebugCheckMathTable(YRTDevice dev, int fn, const uint16_t* table2048, uint64_t* out2);
/* Test-only probe of the device's shading layer (k_check_shade, kernels/k_checks.h): runs the
 * kernels' own BRDF component, CompositedBRDF, camera and light functions on n rows, so that
 * tests can compare them with the reference's classes bit for bit. rows: n x 48 words (wo, Ns, Ng,
 * Tx, Ty, wi, s.xy, ss, component count, 2 pad, 3 x (kind, R.rgb, a, b, c, pad)); out: n x 12
 * words. mode 0: component 0's eval at wi and sample at s (eval, sample, wi, pdf); mode 1: the
 * set's sample at (s, ss) (colour, wi, pdf, type); mode 2: object = a committed camera, pixel =
 * wo.xy, lens = s (org, dir); mode 3: object = a light primitive, P = wo, frame Ns (L, wi, pdf).
 * materials: numMaterials device material records (128 B each) that conductor components index
 * with c; every index in the rows is checked before the launch. Not part of the renderer. */
YRT_API int yrtDebugShade(YRTDevice dev, int mode, YRTHandle object, const float* rows, int n, const void* materials,
                          int numMaterials, float* out);
/* Test-only probe of Material::shade and the texture lookup on the device (k_check_material,
 * k_check_textures, kernels/k_checks.h), on one primitive of a committed, uploaded scene: the
 * primitive's geometry record is read from the scene's uploaded records exactly as k_shade reads
 * it. set: which of the shade kernel's material sets to instantiate ("uber", "obj", "spheres",
 * "stereo", "collada", "all"); a material outside the named set is an error, not a launch.
 * mode 0: rows n x 22 words (wo, Ns, Ng, Tx, Ty, wi, s.xy, dg.s, dg.t), medium4 the current medium
 * (transmission rgb, eta; resolved to the scene's medium index by value), out n x 34 words: the
 * component count, then 3 x (type flags, eval3, sample3, wi3, pdf), zero beyond the count.
 * mode 1: rows n x 2 words (s, t), raw: the material's s0 / ds are not applied; out n x 24 words:
 * RGBA of the lookup through each of the material's texture slots 0..4 (zero where unset), then
 * RGBA of slot 0 through the descriptor copy in the geometry record. Not part of the renderer. */
YRT_API int yrtDebugMaterial(YRTDevice dev, YRTHandle scene, YRTHandle primitive, int mode, const char* set,
                             const float* medium4, const float* rows, int n, float* out);
/* Test-only: the texture tables of a committed scene as the kernels read them. what 0: the image
 * records (24 B: width, height, format, pad, int64 pool offset); 1: the texture records (32 B);
 * 2: the row-major texel pool (8-bit images first); 3: the 2x2 footprint records of the pool's
 * 8-bit part (16 B per texel at 4x the texel's byte offset). Returns the byte count, and copies
 * when buf holds that many; -1 on error. Works on a host-only device too. */
YRT_API int64_t yrtDebugTexturePool(YRTDevice dev, YRTHandle scene, int what, void* buf, size_t bytes);
/* Test-only: the direction-term table of a sample table (kernels/k_sample_dirs.h). The frame
 * cache entry of the request (spp, sets, iteration, num1D, num2D, filter; no lights) is created
 * on the device's first GPU as a render would create it; dims receives its sample table
 * (yrtDebugSampleTable's layout) and dirs4 its table of (cosPhi, sinPhi, cosTheta, sinTheta),
 * [num2D][records] x 4 floats, read back from the device. Returns the record count (sets * spp
 * rounded up to a power of two); a buffer too small for its table is left untouched. */
YRT_API int yrtDebugSampleDirs(YRTDevice dev, int spp, int sets, int iteration, int num1D, int num2D,
                               const char* filter, float* dims, size_t dimsFloats, float* dirs4, size_t dirsFloats);
/* Test-only: the same four terms of n samples (u[i], v[i]) into out4 (n x 4 floats). mode 0: a
 * probe kernel that spells them out per sample as the samplers did before the table; mode 1: the
 * table's own kernel over the samples as one slot of n records. */
YRT_API int yrtDebugDirTerms(YRTDevice dev, int mode, const float* u, const float* v, int n, float* out4);
/* The image tile that logical tile t of a sharded job's frame of T tiles covers
 * (common/yrt_tile_scatter.h: a fixed bijection of [0, T), used by the renderer and the gather
 * whenever the tile stride is above 1). Host-side; -1 for t outside [0, T). */
YRT_API int yrtDebugTileScatter(int t, int T);
/* Test-only probe of the multi-GPU gather's two kernels (k_pack_tiles, k_unpack_tiles,
 * kernels/k_tiles.h), launched exactly as the gathers launch them, on host buffers: fbFloat is
 * numFrames stacked frames of height x width x 3 floats, fbRGB8 the same frames as byte rows of
 * (3 * width rounded up to 4) bytes, slab numTiles * 256 elements (4 bytes each with rgb8, else 16).
 * All three are uploaded; op 0 packs the shard's tiles (job tile = tileOffset + j * tileStride,
 * j < numTiles) and copies the slab back, op 1 unpacks the slab and copies both frame arrays
 * back. Refused without a launch: a host-only device, non-positive sizes, tileOffset < 0,
 * tileStride < 1, an op other than 0 / 1, more tiles than the shard holds, or a host buffer
 * (sizes in bytes) smaller than the job. Not part of the renderer. */
YRT_API int yrtDebugTileSlab(YRTDevice dev, int width, int height, int numFrames, int rgb8, int tileOffset,
                             int tileStride, int numTiles, int op, float* fbFloat, size_t fbFloatBytes,
                             uint8_t* fbRGB8, size_t fbRGB8Bytes, void* slab, size_t slabBytes);
/* The batch plan of a wavefront job over shardTiles tiles at spp samples per pixel: how a
 * device with `lanes` lanes and a batch capacity of `capacity` paths (yrtSetBatchCapacity)
 * cuts the job into batches. capture != 0: a ray-capture frame (yrtSetRayCapture); grow: the
 * YRT_BATCH_GROW switch. out4 = tiles per batch, batches, paths per batch, lanes used.
 * Host-side (the plan changes speed only, never pixels); -1 on an argument out of range. */
YRT_API int yrtDebugBatchPlan(int64_t shardTiles, int spp, int64_t capacity, int lanes, int capture, int grow,
                              int64_t* out4);
/* Parity debugging: out4 == NULL arms the capture of the per-sample radiance (the pathL terms
 * the resolve sums, in s order) of pixel id y*width+x (-1 disarms) of frame `frame` for the
 * following renders (buffer of maxSamples float4); out4 != NULL copies the captured samples
 * and returns their count (at most maxSamples: the kernel writes no more than the buffer
 * holds). Captures on the device's first GPU only (a multi-GPU device's other GPUs render
 * their tiles uncaptured). Compare with oracle_debug_pixel. */
YRT_API int yrtDebugPixelSamples(YRTDevice dev, int pixelId, int frame, float* out4, int maxSamples);
/* Decoder check: 8-bit pixels of a .jpg/.png in file row order (top row first), before the
 * Image4c flip/requantization of rtNewImageFromFile. Call with out=NULL to get the size. */
YRT_API int yrtDebugDecodeImage(const char* file, int* width, int* height, int* channels, uint8_t* out,
                                size_t outBytes);
YRT_API int yrtDebugSampleTable(int spp, int sets, int iteration, int num1D, int num2D, const char* filter,
                                float* out, size_t outFloats);

#ifdef __cplusplus
}
#endif

#endif /* YRT_DEVICE_H */
