// k_tiles.h — the multi-GPU gather's tile slabs: pack a shard's tiles, unpack them into the frames.
#pragma once

#include "yrt_kernels.h"
#include "../common/yrt_tile_scatter.h"

namespace yrt {

// Slab pixel i of a shard's tile sequence -> (frame f, x, y); frames are numFrames images of
// width x height stacked in memory, tile t = frame t / tilesPerFrame.
__device__ __forceinline__ bool slab_pixel(const SlabLayout& L, int i, int& f, int& x, int& y) {
  const int ntx = (L.width + 15) >> 4;
  int t = L.tileOffset + (i >> 8) * L.tileStride;
  f = t / L.tilesPerFrame;
  t -= f * L.tilesPerFrame;
  if (L.tileStride > 1) t = yrt_tile_scatter(t, L.tilesPerFrame);  // as batch_tile
  x = (t % ntx) * 16 + (i & 15);
  y = (t / ntx) * 16 + ((i >> 4) & 15);
  return x < L.width && y < L.height;
}

// rgb8: the slab holds one 32-bit word per pixel (the RGB8 bytes, what an RGB8 framebuffer
// maps); else float4 (the float pixel, w = the RGB8 bytes)
__global__ __launch_bounds__(256) void k_pack_tiles(const float* __restrict__ fbFloat,
                                                    const uint8_t* __restrict__ fbRGB8, SlabLayout L, int n,
                                                    void* __restrict__ slab) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int f, x, y;
    const bool in = slab_pixel(L, i, f, x, y);
    unsigned c = 0;
    if (in) {
      const uint8_t* p = fbRGB8 + ((size_t)f * L.height + y) * L.rgb8Stride + 3 * x;
      c = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
    if (L.rgb8) {
      ((unsigned*)slab)[i] = c;
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, __uint_as_float(c));
      if (in) {
        const float* fp = fbFloat + (((size_t)f * L.height + y) * L.width + x) * 3;
        v.x = fp[0];
        v.y = fp[1];
        v.z = fp[2];
      }
      ((float4*)slab)[i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_unpack_tiles(const void* __restrict__ slab, float* __restrict__ fbFloat,
                                                      uint8_t* __restrict__ fbRGB8, SlabLayout L, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int f, x, y;
    if (!slab_pixel(L, i, f, x, y)) continue;
    unsigned c;
    if (L.rgb8) {
      c = ((const unsigned*)slab)[i];
    } else {
      const float4 v = ((const float4*)slab)[i];
      float* fp = fbFloat + (((size_t)f * L.height + y) * L.width + x) * 3;
      fp[0] = v.x;
      fp[1] = v.y;
      fp[2] = v.z;
      c = __float_as_uint(v.w);
    }
    uint8_t* o = fbRGB8 + ((size_t)f * L.height + y) * L.rgb8Stride + 3 * x;
    o[0] = (uint8_t)(c & 255u);
    o[1] = (uint8_t)((c >> 8) & 255u);
    o[2] = (uint8_t)((c >> 16) & 255u);
  }
}

}  // namespace yrt
