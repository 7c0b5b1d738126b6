// k_adaptive.h — the check of an adaptive render (device/adaptive.cpp): k_tile_error, the error
// estimate of every tile still active (common/yrt_tile_error.h), and k_tile_compact, which
// rewrites the active-tile list without the tiles the check stopped.
#pragma once

#include "../common/yrt_tile_error.h"
#include "yrt_wave.h"

namespace yrt {

#define YRT_ADAPTIVE_BLOCK 256  // one thread per slot of a tile; the compaction's chunk of the list

// One block per listed tile, one thread per slot: the pixel's term, then the header's tree in LDS
// (no atomics: the sum's order is fixed). Thread 0 stores E_T and the tile's iteration count under
// the image tile and the stop flag under the tile's place in the list.
__global__ __launch_bounds__(YRT_ADAPTIVE_BLOCK) void k_tile_error(const float4* __restrict__ accu,
                                                                   const float4* __restrict__ half, int width,
                                                                   int height, int numTilesX,
                                                                   const int* __restrict__ list, int count,
                                                                   float threshold, int iterations,
                                                                   float* __restrict__ tileError,
                                                                   int* __restrict__ tileIterations,
                                                                   int* __restrict__ stopped) {
  __shared__ float slots[YRT_TILE_ERROR_SLOTS];
  const int j = blockIdx.x;
  if (j >= count) return;
  const int tile = list[j];
  const int ty = tile / numTilesX, tx = tile - ty * numTilesX;
  const int k = threadIdx.x;
  const int x = tx * 16 + (k & 15), y = ty * 16 + (k >> 4);
  float e = 0.0f;
  if (x < width && y < height) {
    const size_t pix = (size_t)y * width + x;
    const float4 S = accu[pix], H = half[pix];
    const float s4[4] = {S.x, S.y, S.z, S.w}, h4[4] = {H.x, H.y, H.z, H.w};
    e = yrt_pixel_error(s4, h4);
  }
  slots[k] = e;
  __syncthreads();
  for (int h = YRT_TILE_ERROR_SLOTS / 2; h >= 1; h >>= 1) {
    if (k < h) yrt_tile_tree_step(slots, k, h);
    __syncthreads();
  }
  if (k == 0) {
    const float E = yrt_tile_error_mean(slots[0], yrt_tile_pixels(tx, ty, width, height));
    tileError[tile] = E;
    tileIterations[tile] = iterations;
    stopped[j] = E < threshold ? 1 : 0;  // strict; a NaN never stops
  }
}

// the block's count of p over its threads, to every thread (sums[] one word per wave)
__device__ __forceinline__ unsigned block_count(bool p, unsigned* sums, unsigned& below) {
  const unsigned long long m = ballot(p);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) sums[wave] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned total = 0, before = 0;
  for (int w = 0; w < YRT_ADAPTIVE_BLOCK / 64; ++w) {
    before += w < wave ? sums[w] : 0u;
    total += sums[w];
  }
  __syncthreads();  // sums is reused by the caller's next count
  below = before + lanes_below(m);
  return total;
}

// Stable compaction of the list: block b owns entries [b * 256, b * 256 + 256). Its first output
// slot is the number of survivors before its chunk, which the block counts itself from the stop
// flags (the scan over the blocks: no block waits for another, so the order is the list's own
// whatever the blocks' timing); inside the chunk a ballot and a prefix sum place the survivors.
// The block of the last chunk stores the new count.
__global__ __launch_bounds__(YRT_ADAPTIVE_BLOCK) void k_tile_compact(const int* __restrict__ listIn,
                                                                     const int* __restrict__ stopped, int count,
                                                                     int* __restrict__ listOut,
                                                                     int* __restrict__ countOut) {
  __shared__ unsigned sums[YRT_ADAPTIVE_BLOCK / 64];
  const int first = blockIdx.x * YRT_ADAPTIVE_BLOCK;
  if (first >= count) return;
  unsigned base = 0, below = 0;
  for (int at = 0; at < first; at += YRT_ADAPTIVE_BLOCK)  // first is a multiple of the block: whole chunks
    base += block_count(stopped[at + (int)threadIdx.x] == 0, sums, below);
  const int j = first + (int)threadIdx.x;
  const bool keep = j < count && stopped[j] == 0;
  const unsigned kept = block_count(keep, sums, below);
  if (keep) listOut[base + below] = listIn[j];
  if (threadIdx.x == 0 && first + YRT_ADAPTIVE_BLOCK >= count) *countOut = (int)(base + kept);
}

}  // namespace yrt
