// yrt_wave.h — what every kernel of the wavefront path tracer shares: wave-wide ballot / append
// helpers, the segmented-queue map, the reference's random number generator and hashes,
// constant-address-space loads, and the profile builds' counters.
//
// Wave64: every cross-lane primitive below is written for 64 lanes (ballot is 64-bit).
#pragma once

#include <hip/hip_runtime.h>

#include "yrt_kernels.h"

namespace yrt {

#ifndef YRT_BLOCK
#define YRT_BLOCK 64  // raygen / shade / resolve blocks: one wave (128: +0.5 %, 64: +0.9 % over 256, two lanes)
#endif

// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ int lane_id() { return __lane_id(); }
// 0.0f computed where it is used (volatile: not hoisted out of a loop)
__device__ __forceinline__ float opaque_zero() {
  float z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}
// set bits of a wave mask below this lane (v_mbcnt: no per-lane mask register kept live)
__device__ __forceinline__ unsigned lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Ballot of a bool (the builtin on the i1 lane mask; HIP's __ballot takes an int).
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ unsigned wave_append(unsigned* counter, bool pred, bool& got) {
  const unsigned long long mask = ballot(pred);
  got = pred;
  if (mask == 0) return 0;
  const int lane = lane_id();
  const int leader = __ffsll((long long)mask) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
  base = __shfl(base, leader, 64);
  return base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

// Two appends at once: one lane issues both atomics back to back, so the wave waits for the
// slower of the two round trips and not for their sum. Slots as two wave_append calls give them.
__device__ __forceinline__ void wave_append2(unsigned* counter0, bool pred0, unsigned& slot0, unsigned* counter1,
                                             bool pred1, unsigned& slot1) {
  const unsigned long long m0 = ballot(pred0), m1 = ballot(pred1);
  slot0 = slot1 = 0;
  if ((m0 | m1) == 0) return;
  const int lane = lane_id();
  const int leader = __ffsll((long long)(m0 | m1)) - 1;
  unsigned b0 = 0, b1 = 0;
  if (lane == leader) {
    // wave-uniform cases, so that a counter nobody appends to sees no atomic
    if (m0 != 0 && m1 != 0) {
      b0 = atomicAdd(counter0, (unsigned)__popcll(m0));
      b1 = atomicAdd(counter1, (unsigned)__popcll(m1));
    } else if (m0 != 0) {
      b0 = atomicAdd(counter0, (unsigned)__popcll(m0));
    } else {
      b1 = atomicAdd(counter1, (unsigned)__popcll(m1));
    }
  }
  b0 = __shfl(b0, leader, 64);
  b1 = __shfl(b1, leader, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
  slot0 = b0 + (unsigned)__popcll(m0 & below);
  slot1 = b1 + (unsigned)__popcll(m1 & below);
}

// ---------------------------------------------------------------- segmented queues
struct QMap {
  unsigned pre[YRT_QSEGS + 1];  // exclusive prefix of the segment counts; pre[numSegs] = total
};

// Every thread of the block must call it (barrier inside).
__device__ __forceinline__ void qmap_load(QMap& m, const unsigned* counts, int numSegs) {
  if (threadIdx.x == 0) {
    unsigned c[YRT_QSEGS];
#pragma unroll
    for (int k = 0; k < YRT_QSEGS; ++k) c[k] = k < numSegs ? counts[(size_t)k * YRT_QCSTRIDE] : 0u;
    unsigned acc = 0;
#pragma unroll
    for (int k = 0; k < YRT_QSEGS; ++k) {
      m.pre[k] = acc;
      acc += c[k];
    }
    m.pre[YRT_QSEGS] = acc;
  }
  __syncthreads();
}

// Physical slot of logical queue index q < total.
__device__ __forceinline__ int qmap_phys(const QMap& m, int segCap, unsigned q) {
  int lo = 0;
#pragma unroll
  for (int step = YRT_QSEGS / 2; step > 0; step >>= 1)
    if (m.pre[lo + step] <= q) lo += step;
  return lo * segCap + (int)(q - m.pre[lo]);
}

// Segment that input item q appends into (uniform across a wave: q >> 6 is).
__device__ __forceinline__ int qseg_of(unsigned q) { return (int)((q >> 6) % YRT_QSEGS); }

// ---------------------------------------------------------------- reference RNG
// Park-Miller minimal standard + Bays-Durham shuffle (common/math/random.h:24-78).
struct DevRandom {
  int seed, state;
  int table[32];
  __device__ void setSeed(int s) {
    const int a = 16807, m = 2147483647, q = 127773, r = 2836;
    if (s == 0) seed = 1;
    else if (s < 0) seed = -s;
    else seed = s;
    for (int j = 32 + 7; j >= 0; j--) {
      int k = seed / q;
      seed = a * (seed - k * q) - r * k;
      if (seed < 0) seed += m;
      if (j < 32) table[j] = seed;
    }
    state = table[0];
  }
  __device__ int getInt() {
    const int a = 16807, m = 2147483647, q = 127773, r = 2836;
    int k = seed / q;
    seed = a * (seed - k * q) - r * k;
    if (seed < 0) seed += m;
    int j = state / (1 + (2147483647 - 1) / 32);
    state = table[j];
    table[j] = seed;
    return state;
  }
  __device__ int getInt(int limit) { return getInt() % limit; }
  __device__ float getFloat() { return fminf(getInt() / 2147483647.0f, 1.0f - kUlp); }
};

// Counter-based replacement for C rand() in the shadow-ray jitter
// (pathtraceintegrator.cpp:151; the reference calls rand() from worker threads, so it
// is not reproducible). Same function in oracle/yrt_oracle.c: hash_u01.
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16; h *= 0x7feb352dU; h ^= h >> 15; h *= 0x846ca68bU; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ float hash_u01(uint32_t seed, uint32_t pixel, uint32_t sample, uint32_t depthLight) {
  uint32_t h = mix32(seed ^ 0x9e3779b9U);
  h = mix32(h ^ pixel);
  h = mix32(h ^ (sample * 0x85ebca6bU));
  h = mix32(h ^ (depthLight * 0xc2b2ae35U));
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// Records every lane of a wave reads at one address (the render parameters, the frame's
// camera) are read through the constant address space: scalar loads into SGPRs instead of
// per-lane vector loads held in VGPRs (the kernels never write them).
#define YRT_CONST __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const YRT_CONST T& const_ref(const T* p) {
  return *(const YRT_CONST T*)p;
}

template <class F>
__device__ __forceinline__ V3 ld3(const F* p) { return v3(p[0], p[1], p[2]); }
__device__ __forceinline__ V3 ld3(const float4& p) { return v3(p.x, p.y, p.z); }
template <class F>
__device__ __forceinline__ A3 ldA3(const F* m) {
  return a3(l3(v3(m[0], m[1], m[2]), v3(m[3], m[4], m[5]), v3(m[6], m[7], m[8])), v3(m[9], m[10], m[11]));
}

// ---------------------------------------------------------------- profile counters
#if defined(YRT_PROFILE) && defined(YRT_SHADE_PROF)
#error "YRT_PROFILE and YRT_SHADE_PROF share the profile counters: build one at a time"
#endif
#if defined(YRT_PROFILE) || defined(YRT_SHADE_PROF)
// YRT_PROFILE: [0] outer iterations x waves, [1] lanes holding a ray at outer iterations,
// [2] node-phase iterations, [3] lanes visiting a node, [4] leaf passes with work,
// [5] triangle-loop iterations (max leaf size per pass), [6] useful triangle tests
// YRT_SHADE_PROF: [0..6] k_shade shader-clock cycles per phase summed over waves, [7] wave
// iterations (see k_shade)
__device__ unsigned long long g_traceProfile[8];
#endif

}  // namespace yrt
