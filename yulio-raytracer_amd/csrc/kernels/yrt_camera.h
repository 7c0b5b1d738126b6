// yrt_camera.h — the camera models (pinhole, depth of field, stereo cube) and the mapping of a
// batch's pixel index to its frame and image pixel; shared by k_raygen, the fused depth-0
// k_trace, k_shade, k_resolve_pixels, k_debug and k_pick.
#pragma once

#include "../common/yrt_tile_scatter.h"
#include "yrt_wave.h"

namespace yrt {

// ---------------------------------------------------------------- cameras
// PinHoleCamera::ray (cameras/pinholecamera.h:23-25)
// StereoCubeCamera::ray (cameras/StereoCubeCamera.h:68-161)
// DepthOfFieldCamera::ray (cameras/depthoffieldcamera.h:20-26); (lx, ly) = the lens sample
template <class CAM>
__device__ __forceinline__ void pinhole_ray(const CAM& cam, float fx, float fy, V3& org, V3& dir) {
  A3 p2w = ldA3(cam.p2w[0]);
  org = p2w.p;
  dir = normalize(fx * p2w.l.vx + (1.0f - fy) * p2w.l.vy + p2w.l.vz);
}
// TOEIN = false drops the toe-in stereo branch: the fused depth-0 trace kernel takes no toe-in
// camera (the host routes those frames through k_raygen). Its two rotations about per-ray
// points and the reference's rcp/rsqrt sequences need ~40 more VGPRs than the rest of the
// camera code (k_raygen 37 -> 76), which at the fused kernel's 96-VGPR cap spilled 60-76 B
// into its traversal loop.
template <bool TOEIN = true, class CAM>  // GpuCamera, or a YRT_CONST one (scalar loads)
__device__ void camera_ray(const CAM& cam, float fx, float fy, V3& org, V3& dir, float lx = 0.f,
                           float ly = 0.f) {
  if (cam.type == CAM_PINHOLE) {
    pinhole_ray(cam, fx, fy, org, dir);
    return;
  }
  if (cam.type == CAM_DOF) {
    const A3 p2w = ldA3(cam.p2w[0]), l2w = ldA3(cam.p2w[1]);
    const float lensRadius = cam.xyzStraight[0], focalDistance = cam.xyzStraight[1];
    // uniformSampleDisk (samplers/shapesampler.h:187-191)
    const float r = sqrtf(lx), theta = kTwoPi * ly;
    const V3 begin = xfmPoint(l2w, v3(lensRadius * r * yrt_cosf(theta), lensRadius * r * yrt_sinf(theta), 0.0f));
    const V3 end = p2w.p + focalDistance * (fx * p2w.l.vx + (1.0f - fy) * p2w.l.vy + p2w.l.vz);
    org = begin;
    dir = normalize(end - begin);
    return;
  }
  const A3 pixel2world = ldA3(cam.p2w[0]);
  const int eyeCubeFaceIndex = cam.cubeFaceIndex % 6;
  const float yPixel = 1.0f - fy;
  A3 p2w = ldA3(cam.p2w[eyeCubeFaceIndex]);
  const V3 xyzStraight = ld3(cam.xyzStraight);
  float theta = 0.f;
  float absoluteVerticalAngle = 0.f;
  if (eyeCubeFaceIndex <= 3) {
    const V3 xDir = normalize(fx * pixel2world.l.vx + .5f * pixel2world.l.vy + pixel2world.l.vz);
    theta = yrt_acosf(clampf(dot(xDir, xyzStraight), -1.f, 1.f)) * signf_(fx - .5f);
    const V3 yDir = normalize(.5f * pixel2world.l.vx + yPixel * pixel2world.l.vy + pixel2world.l.vz);
    const float yAngle = rad2deg(yrt_acosf(clampf(dot(yDir, xyzStraight), -1.f, 1.f))) * signf_(yPixel - .5f);
    absoluteVerticalAngle = fabsf(yAngle);
  } else {
    const V3 xyDir = v3(fx - .5f, yPixel - .5f, 0.f);
    const V3 xyDirNorm = normalize(xyDir);
    const V3 xyUp = v3(0.f, eyeCubeFaceIndex == 4 ? -1.f : 1.f, 0.f);
    theta = yrt_acosf(clampf(dot(xyDirNorm, xyUp), -1.f, 1.f)) * signf_(fx - .5f);
    const V3 xyzDir = normalize(fx * pixel2world.l.vx + yPixel * pixel2world.l.vy + pixel2world.l.vz);
    const float xyzAngle = rad2deg(yrt_acosf(clampf(dot(xyzDir, xyzStraight), -1.f, 1.f)));
    absoluteVerticalAngle = 90.f - fabsf(xyzAngle);
  }
  float eyeOffset = cam.eyeSeparation * (cam.cubeFaceIndex < 6 ? -.5f : .5f);
  if (absoluteVerticalAngle > cam.falloffAngle) {
    const float coef = 1.f - smoothstepf(0.f, 1.f, smoothstepf(cam.falloffAngle, 90.f, absoluteVerticalAngle));
    eyeOffset *= coef;
  }
  if (TOEIN && cam.toeIn) {
    p2w = mul(p2w, a3_translate(v3(eyeOffset, 0.f, 0.f)));
    const V3 origin = ld3(cam.origin), up = ld3(cam.up);
    const A3 rayRotationSpace = a3_rotate_about(origin, up, theta);
    const V3 rayOrigin = mul(rayRotationSpace, p2w).p;
    const float toeInCorrection = -yrt_atanf(eyeOffset * cam.rcpZeroParallaxDistance);
    p2w = mul(a3_rotate_about(rayOrigin, up, toeInCorrection), p2w);
    org = rayOrigin;
    dir = normalize(fx * p2w.l.vx + yPixel * p2w.l.vy + p2w.l.vz);
    return;
  }
  // Without toe-in the same products with the pixel-independent terms taken from the camera
  // record (objects.cpp): translate(origin) * rotate(up, theta) * translate(-origin) has the
  // rotation as its linear part (the identity factors' ones and zeros only add exact zeros),
  // and its point is rotation * (-origin) + rotP; the shifted eye point is
  // p2w.p + eyeOffset * p2w.vx plus the translation's zero products.
  const auto* R = cam.rot;  // u.xyz, uxx, 1-uxx, uyy, 1-uyy, uzz, 1-uzz, uxy, uxz, uyz
  const float sn = yrt_sinf(theta), cs = yrt_cosf(theta), omc = 1 - cs;
  const V3 rvx = v3(R[3] + R[4] * cs, R[9] * omc + R[2] * sn, R[10] * omc - R[1] * sn);
  const V3 rvy = v3(R[9] * omc - R[2] * sn, R[5] + R[6] * cs, R[11] * omc + R[0] * sn);
  const V3 rvz = v3(R[10] * omc + R[1] * sn, R[11] * omc - R[0] * sn, R[7] + R[8] * cs);
  // the rotation's products through the fused LinearSpace3 * v helper, as the oracle's lmul
  const L3 rot = l3(rvx, rvy, rvz);
  const V3 bp = mul(rot, ld3(cam.negO)) + ld3(cam.rotP);
  const auto* z = cam.zero[eyeCubeFaceIndex];
  const V3 eye = v3(eyeOffset * p2w.l.vx.x + z[0], eyeOffset * p2w.l.vx.y + z[1], eyeOffset * p2w.l.vx.z + z[2]) + p2w.p;
  org = mul(rot, eye) + bp;
  const auto* m = cam.lin[eyeCubeFaceIndex];
  dir = normalize(fx * v3(m[0], m[1], m[2]) + yPixel * v3(m[3], m[4], m[5]) + v3(m[6], m[7], m[8]));
}

// ---------------------------------------------------------------- batch pixel mapping
// Batch pixel i -> (frame f, pixel x, y). A batch holds whole 16x16 tiles of the job's tile
// sequence (all frames' tiles, frame-major); the 256 pixels of a tile are consecutive, so the
// 64 lanes of a wave (64-aligned i) always share the tile and the frame.
template <class D>  // FastDiv, or a YRT_CONST one
__device__ __forceinline__ int fastdiv(int n, const D& d) {  // n in [0, 2^31)
  return (int)((__umulhi((unsigned)n, d.mul) + (unsigned)n) >> d.shift);
}
// the tile of batch-pixel block ib = i >> 8: its frame and first pixel (false past the job).
// tileList (PathBuffers::reserved) != null: a batch of an adaptive render (device/adaptive.cpp),
// whose tiles are the image tiles tileList[firstTile + ib] of one unsharded frame (ib below the
// batch's tiles: the list ends with the last batch).
template <class RP>
__device__ __forceinline__ bool batch_tile(const RP& rp, const BatchInfo& bi, int ib, int& x0, int& y0,
                                           int& f, const int* tileList = nullptr) {
  f = 0;
  if (tileList) {
    const int t = tileList[bi.firstTile + ib];
    const int ty = fastdiv(t, rp.divTilesX);
    x0 = (t - ty * rp.numTilesX) * 16;
    y0 = ty * 16;
    return true;
  }
  int tile = bi.tileOffset + (bi.firstTile + ib) * bi.tileStride;
  if (tile >= rp.tilesPerFrame * rp.numFrames) return false;
  if (rp.numFrames > 1) {
    f = fastdiv(tile, rp.divTilesPerFrame);
    tile -= f * rp.tilesPerFrame;
  }
  // sharded jobs: the logical tile's image tile (common/yrt_tile_scatter.h; slab_pixel agrees)
  if (bi.tileStride > 1) tile = yrt_tile_scatter(tile, rp.tilesPerFrame);
  const int ty = fastdiv(tile, rp.divTilesX);
  x0 = (tile - ty * rp.numTilesX) * 16;
  y0 = ty * 16;
  return true;
}
template <class RP>
__device__ __forceinline__ bool batch_pixel(const RP& rp, const BatchInfo& bi, int i, int& x, int& y,
                                            int& f, const int* tileList = nullptr) {
  int x0 = 0, y0 = 0;
  if (!batch_tile(rp, bi, i >> 8, x0, y0, f, tileList)) return false;
  x = x0 + (i & 15);
  y = y0 + ((i >> 4) & 15);
  return x < rp.width && y < rp.height;
}
template <class RP>
__device__ __forceinline__ bool batch_pixel(const RP& rp, const BatchInfo& bi, int i, int& x, int& y,
                                            const int* tileList = nullptr) {
  int f;
  return batch_pixel(rp, bi, i, x, y, f, tileList);
}

__device__ __forceinline__ float samp(const FrameView& fv, int dim, int rec) {
  return fv.samples[(size_t)dim * fv.numRecords + rec];
}
// the tabulated direction terms (sample_dir, yrt_shade.h) of record rec's 2-D sample `slot`
__device__ __forceinline__ float4 samp_dir(const FrameView& fv, int slot, int rec) {
  return fv.sampleDirs[(size_t)slot * fv.numRecords + rec];
}

}  // namespace yrt
