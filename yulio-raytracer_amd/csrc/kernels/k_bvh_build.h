// k_bvh_build.h — the kernels of the scene builder "morton": one thread per element, 64-thread
// blocks, every step one of common/yrt_lbvh.h's and yrt_bvh4.h's functions (the host loop of
// device/bvh_build.cpp calls the same ones). No kernel reads what another workgroup of the same
// launch wrote: a kernel boundary is the only hand-over (the XCDs' L2s are private), nothing polls
// or waits, and the only atomics are reductions (centroid bounds, flags, the stack bound) that the
// next launch or the host reads. Every index used as an address derives from N, which the host
// checked.
#pragma once

#include <hip/hip_runtime.h>

#include "../common/yrt_lbvh.h"

namespace yrt {

#define YRT_LBVH_BLOCK 64

// float <-> unsigned with the same order, for atomicMin / atomicMax
__device__ __forceinline__ unsigned lbvh_ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lbvh_unordered(unsigned e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// state words shared by the launches of one build
struct LbvhState {
  unsigned cbLo[3], cbHi[3];  // centroid bounds, lbvh_ordered (start: ~0 / 0)
  int nonFinite;              // a vertex or box centre is not finite
  int tooDeep;                // a radix-tree node below YRT_LBVH_MAX_LEVELS levels
  int maxStack;               // worst-case traversal stack so far
  int nextCount;              // inner children of the collapse level just emitted
  int numLevels;              // radix-tree levels with inner nodes
  int levelStart[YRT_LBVH_MAX_LEVELS + 1];
};

// 1 boxes and centroid bounds
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_prims(const float* __restrict__ v, const float* __restrict__ v1,
                                                              int N, Box* __restrict__ primBox,
                                                              LbvhState* __restrict__ st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  Box cb;  // this lane's part of the centroid bounds: empty, or its box centre
  cb.reset();
  bool bad = false;
  if (i < N) {
    Box b;
    bad = !lbvh_prim_box(v + (size_t)i * 9, v1 ? v1 + (size_t)i * 9 : nullptr, b);
    primBox[i] = b;
    for (int k = 0; k < 3; ++k) cb.lo[k] = cb.hi[k] = b.centre(k);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    Box o;
    for (int k = 0; k < 3; ++k) { o.lo[k] = __shfl_xor(cb.lo[k], m); o.hi[k] = __shfl_xor(cb.hi[k], m); }
    cb.grow(o);
  }
  const bool anyBad = __any(bad);
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 3; ++k) {
      // a NaN centre is flagged, and never compared on: the bounds of a flagged scene are not used
      atomicMin(&st->cbLo[k], lbvh_ordered(cb.lo[k]));
      atomicMax(&st->cbHi[k], lbvh_ordered(cb.hi[k]));
    }
    if (anyBad) atomicOr(&st->nonFinite, 1);
  }
}

// 2 keys
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_keys(const Box* __restrict__ primBox,
                                                             const LbvhState* __restrict__ st, int N,
                                                             uint64_t* __restrict__ keys, uint32_t* __restrict__ ids) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Box cb;
  for (int k = 0; k < 3; ++k) { cb.lo[k] = lbvh_unordered(st->cbLo[k]); cb.hi[k] = lbvh_unordered(st->cbHi[k]); }
  keys[i] = lbvh_key(primBox[i], cb);
  ids[i] = (uint32_t)i;
}

// 3, 4 hierarchy and leaves: node i of N - 1; parent[] starts at -1 and is written for inner children
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_hierarchy(const uint64_t* __restrict__ keys, int N,
                                                                  Node2* __restrict__ nodes,
                                                                  int* __restrict__ parent, int* __restrict__ inner) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N - 1) return;
  int first, last, split;
  lbvh_range(keys, N, i, first, last, split);
  const bool in = lbvh_is_inner(i, first, last);
  inner[i] = in ? 1 : 0;
  if (!in) return;
  Node2 n;
  lbvh_node2(first, last, split, n);
  for (int c = 0; c < 2; ++c) {
    nodes[i].idx[c] = n.idx[c];
    nodes[i].cnt[c] = n.cnt[c];
    if (n.cnt[c] == 0) parent[n.idx[c]] = i;
  }
}

// levels, top-down by the parent links of the launch before: sort key = depth, 255 for nodes
// that are not part of the tree
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_depth(const int* __restrict__ parent,
                                                              const int* __restrict__ inner, int count,
                                                              uint32_t* __restrict__ depth, uint32_t* __restrict__ node,
                                                              LbvhState* __restrict__ st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  node[i] = (uint32_t)i;
  if (!inner[i]) { depth[i] = 255u; return; }
  int d = 0;
  for (int p = parent[i]; p >= 0 && d < YRT_LBVH_MAX_LEVELS; p = parent[p]) ++d;
  if (d >= YRT_LBVH_MAX_LEVELS) {
    atomicOr(&st->tooDeep, 1);
    d = YRT_LBVH_MAX_LEVELS - 1;
  }
  depth[i] = (uint32_t)d;
}

// the per-level lists are the runs of the nodes sorted by depth
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_level_starts(const uint32_t* __restrict__ depth, int count,
                                                                     LbvhState* __restrict__ st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int d = (int)depth[i], prev = i > 0 ? (int)depth[i - 1] : -1;
  if (d != prev) {
    if (d < 255) {
      st->levelStart[d] = i;
    } else {
      st->levelStart[prev + 1] = i;
      st->numLevels = prev + 1;
    }
  }
  if (i == count - 1 && d < 255) {
    st->levelStart[d + 1] = count;
    st->numLevels = d + 1;
  }
}

// 5 boxes of one level (deepest first)
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_boxes(Node2* __restrict__ nodes,
                                                              const Box* __restrict__ primBox,
                                                              const uint32_t* __restrict__ slotId,
                                                              const uint32_t* __restrict__ levelNodes, int count) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int i = (int)levelNodes[t];
  for (int c = 0; c < 2; ++c) {
    Box b;
    lbvh_child_box(nodes, primBox, slotId, i, c, b);
    nodes[i].b[c] = b;
  }
}

// 6, 7 collapse of one 4-wide level: count the inner children, (scan,) emit
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_count(const Node2* __restrict__ nodes,
                                                              const int* __restrict__ frontier, int count,
                                                              int* __restrict__ numInner) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= count) return;
  Ref ch[4];
  const int k = collapse4(nodes, frontier[f], ch);
  numInner[f] = lbvh_count_inner(ch, k);
}

// node base + f; its inner children are nodes base + count + off[f] ..; cap: entries of next / nextStack
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_emit(const Node2* __restrict__ nodes,
                                                             const int* __restrict__ frontier,
                                                             const int* __restrict__ stackAbove,
                                                             const int* __restrict__ off, int count, int base,
                                                             GpuNode* __restrict__ out, int* __restrict__ next,
                                                             int* __restrict__ nextStack, int cap,
                                                             LbvhState* __restrict__ st) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= count) return;
  Ref ch[4];
  const int k = collapse4(nodes, frontier[f], ch);
  const int stackHere = stackAbove[f] + (k - 1);
  atomicMax(&st->maxStack, stackHere);
  int node[4], nx[4];
  const int ni = lbvh_number(ch, k, base + count + off[f], node, nx);
  GpuNode g;
  write_node4(g, ch, k, node);
  out[base + f] = g;
  for (int r = 0; r < ni; ++r)
    if (off[f] + r < cap) { next[off[f] + r] = nx[r]; nextStack[off[f] + r] = stackHere; }
  if (f == count - 1) st->nextCount = off[f] + ni;
}

// 9 leaf records
__global__ __launch_bounds__(YRT_LBVH_BLOCK) void k_lbvh_leaves(const float* __restrict__ v,
                                                               const uint32_t* __restrict__ flags,
                                                               const uint32_t* __restrict__ slotId, int N,
                                                               GpuTri* __restrict__ tris) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  GpuTri g;
  write_leaf_record(g, v, flags, slotId[i]);
  tris[i] = g;
}

}  // namespace yrt
