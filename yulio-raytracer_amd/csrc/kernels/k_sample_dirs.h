// k_sample_dirs.h — the direction-term table of a frame's sample table, and its test probe.
#pragma once

#include "yrt_shade.h"

namespace yrt {

// out[slot * numRecords + rec] = sample_dir(u, v) of record rec's 2-D sample `slot`. pairs: the
// 2-D rows of the sample table, [2 * numSlots][numRecords] (u row, then v row, per slot). Runs
// once per uploaded table (FrameCache), so k_shade loads what it evaluated per vertex before:
// the same device functions on the same inputs, hence the same bits.
__global__ __launch_bounds__(256) void k_sample_dirs(const float* __restrict__ pairs, int numRecords, int numSlots,
                                                     float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numSlots * numRecords) return;
  const int slot = i / numRecords, rec = i - slot * numRecords;
  const float u = pairs[(size_t)(2 * slot) * numRecords + rec];
  const float v = pairs[(size_t)(2 * slot + 1) * numRecords + rec];
  out[i] = sample_dir(u, v);
}

// Test probe (yrtDebugDirTerms mode 0): the terms of n samples (u[i], v[i]) spelled out as the
// samplers evaluated them per vertex before the table, without sample_dir.
__global__ __launch_bounds__(64) void k_check_dir_terms(const float* __restrict__ u, const float* __restrict__ v, int n,
                                                        float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float phi = kTwoPi * u[i];
  const float cosTheta = sqrtf(v[i]), sinTheta = sqrtf(1.0f - v[i]);
  out[i] = make_float4(yrt_cosf(phi), yrt_sinf(phi), cosTheta, sinTheta);
}

}  // namespace yrt
