// yrt_bvh4.h — from a binary tree to the 4-wide 128-B nodes and the leaf records of
// yrt_gpu_types.h, written once for every builder: the host SAH builders and the host loop of the
// scene builder "morton" (device/bvh_build.cpp) and its kernels (kernels/k_bvh_build.h) call these
// functions, so they agree on the box, the child reference, the collapse rule, the node's bytes
// and a leaf record's bytes by construction (-ffp-contract=off on both sides; comparisons instead
// of fmin / fmax, so that +0 / -0 and the operand order are spelled out).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "yrt_gpu_types.h"
#include "yrt_tri_record.h"

// member functions: YRT_THD without the `static`
#if defined(__HIPCC__)
#define YRT_MHD __host__ __device__ __forceinline__
#else
#define YRT_MHD inline
#endif

namespace yrt {

struct Box {
  float lo[3], hi[3];
  // the empty box: growing it by b gives b, its area is 0
  YRT_MHD void reset() {
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
  }
  YRT_MHD void grow(const Box& b) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = b.lo[k] < lo[k] ? b.lo[k] : lo[k];
      hi[k] = b.hi[k] > hi[k] ? b.hi[k] : hi[k];
    }
  }
  YRT_MHD void growP(const float* p) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = p[k] < lo[k] ? p[k] : lo[k];
      hi[k] = p[k] > hi[k] ? p[k] : hi[k];
    }
  }
  YRT_MHD float centre(int k) const { return 0.5f * (lo[k] + hi[k]); }
  // surface area; 0 for a box that is inverted (or has a NaN) on an axis
  YRT_MHD float area() const {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.f;
    return 2.f * (dx * dy + dy * dz + dz * dx);
  }
};
YRT_THD Box intersect(const Box& a, const Box& b) {
  Box r;
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = a.lo[k] < b.lo[k] ? b.lo[k] : a.lo[k];
    r.hi[k] = b.hi[k] < a.hi[k] ? b.hi[k] : a.hi[k];
  }
  return r;
}

// A child of a binary node: cnt 0: the inner binary node idx; cnt > 0: the leaf of the leaf
// slots [idx, idx + cnt)
struct Ref {
  Box b;
  int idx, cnt;
};
struct Node2 {
  Box b[2];
  int idx[2], cnt[2];
  YRT_MHD Ref child(int j) const { return Ref{b[j], idx[j], cnt[j]}; }
  YRT_MHD void set(int j, const Ref& r) { b[j] = r.b; idx[j] = r.idx; cnt[j] = r.cnt; }
};

// The children of the 4-wide node made from binary node n2: its two children; then, until there
// are four, the inner child of the largest area (ties: the lowest slot) is opened, its left child
// takes the slot and its right child the next free one. Returns the child count (2 .. 4).
YRT_THD int collapse4(const Node2* in, int n2, Ref ch[4]) {
  int k = 2;
  for (int j = 0; j < 2; ++j) ch[j] = in[n2].child(j);
  while (k < 4) {
    int best = -1;
    float bestArea = -1.f;
    for (int j = 0; j < k; ++j) {
      if (ch[j].cnt != 0) continue;
      const float a = ch[j].b.area();
      if (a > bestArea) { bestArea = a; best = j; }
    }
    if (best < 0) break;
    const Node2& o = in[ch[best].idx];
    ch[best] = o.child(0);
    ch[k++] = o.child(1);
  }
  return k;
}

// The 128-B node of children ch[0 .. k): the 24 planes, the pad, and the child words: a leaf as
// (slot << 5) | count, an inner child as node[j] << 5, where node[j] is the index that the caller's
// numbering gave it (read for inner children only). An empty slot gets -1 and an inverted infinite
// box (lo = +inf, hi = -inf): with sign-ordered slab planes its entry distance is +inf and its
// exit -inf for every ray, so the trace kernels cull it without testing the child word (which
// stays -1 for the other traversals).
YRT_THD void write_node4(GpuNode& g, const Ref ch[4], int k, const int node[4]) {
  for (int j = 0; j < 4; ++j) {
    const bool v = j < k;
    const float L = INFINITY, H = -INFINITY;
    g.lox[j] = v ? ch[j].b.lo[0] : L; g.hix[j] = v ? ch[j].b.hi[0] : H;
    g.loy[j] = v ? ch[j].b.lo[1] : L; g.hiy[j] = v ? ch[j].b.hi[1] : H;
    g.loz[j] = v ? ch[j].b.lo[2] : L; g.hiz[j] = v ? ch[j].b.hi[2] : H;
    g.child[j] = !v ? -1 : ((ch[j].cnt ? ch[j].idx : node[j]) << 5) | ch[j].cnt;
    g.pad[j] = 0;
  }
}

// The leaf record of triangle id (v: 9 floats per triangle id): the t = 0 triangle, v0.w = id,
// e1.w = flags[id], e2.w = 0 (the geometry id is scene_gpu.cpp's to fill in).
YRT_THD void write_leaf_record(GpuTri& g, const float* v, const uint32_t* flags, uint32_t id) {
  const float* t = v + (size_t)id * 9;
  yrt_tri_vertices(g, t, t + 3, t + 6);
  union { uint32_t u; float f; } a, b;
  a.u = id;
  b.u = flags[id];
  g.v0[3] = a.f;
  g.e1[3] = b.f;
  g.e2[3] = 0.f;
}

}  // namespace yrt
