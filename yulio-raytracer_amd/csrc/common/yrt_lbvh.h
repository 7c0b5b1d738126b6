// yrt_lbvh.h — the per-element steps of the "morton" scene builder (LBVH, Karras 2012, collapsed
// to 4-wide nodes), written once: the kernels of kernels/k_bvh_build.h and the serial host loop of
// device/bvh_build.cpp call the same functions, so both give the same bytes (-ffp-contract=off on
// both sides, comparisons instead of fmin / fmax so that +0 / -0 and the operand order are spelled
// out), as yrt_qnode.h and yrt_tri_record.h do for the quantizer and the leaf records.
//
//   1 lbvh_prim_box     vertex bounds of a triangle (both ends of the frame time), finiteness
//   2 lbvh_key          63-bit Morton code of the box centre inside the centroid bounds
//   3 lbvh_range        node i of the N - 1 radix-tree nodes: its key range and split
//     lbvh_node2        the node's two child references; a range of <= YRT_MAX_LEAF keys is a leaf
//   5 lbvh_child_box    a child's box, bottom-up: the exact union of its triangles' / its node's boxes
//   6 lbvh_collapse     Collapser::collapse's rule for one 4-wide node (device/bvh_build.cpp)
//     lbvh_emit         the 128-B node
//   9 lbvh_leaf_record  the leaf record of a sorted slot
#pragma once

#include <math.h>
#include <stdint.h>

#include "yrt_gpu_types.h"
#include "yrt_tri_record.h"

#ifndef YRT_MAX_LEAF
#define YRT_MAX_LEAF 8
#endif
// levels of the radix tree the build can hold: 63 key bits + 32 index bits (equal keys) bound it
#define YRT_LBVH_MAX_LEVELS 128

namespace yrt {

struct LbvhBox {
  float lo[3], hi[3];
};

// A radix-tree node as the collapse reads it (bvh_build.cpp Node2): cnt 0: inner node idx;
// cnt > 0: the leaf of sorted slots [idx, idx + cnt)
struct LbvhNode2 {
  LbvhBox b[2];
  int idx[2], cnt[2];
};

struct LbvhRef {
  LbvhBox b;
  int idx, cnt;
};

YRT_THD void lbvh_box_reset(LbvhBox& b) {
  for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
}
YRT_THD void lbvh_box_grow(LbvhBox& a, const LbvhBox& b) {
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k];
    a.hi[k] = b.hi[k] > a.hi[k] ? b.hi[k] : a.hi[k];
  }
}
// Box::area of bvh_build.cpp
YRT_THD float lbvh_box_area(const LbvhBox& b) {
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.f;
  return 2.f * (dx * dy + dy * dz + dz * dx);
}

// ---------------------------------------------------------------- 1 primitive box
// v, v1: the triangle's 9 floats at time 0 and (moving scenes, else null) time 1. Returns false
// when a coordinate or the box centre is not finite.
YRT_THD bool lbvh_prim_box(const float* v, const float* v1, LbvhBox& b) {
  lbvh_box_reset(b);
  bool ok = true;
  for (int s = 0; s < 2; ++s) {
    const float* p = s ? v1 : v;
    if (!p) continue;
    for (int j = 0; j < 9; ++j) {
      const float x = p[j];
      const int k = j % 3;
      ok = ok && (x - x == 0.f);
      b.lo[k] = x < b.lo[k] ? x : b.lo[k];
      b.hi[k] = x > b.hi[k] ? x : b.hi[k];
    }
  }
  for (int k = 0; k < 3; ++k) {
    const float c = 0.5f * (b.lo[k] + b.hi[k]);
    ok = ok && (c - c == 0.f);
  }
  return ok;
}
YRT_THD float lbvh_centroid(const LbvhBox& b, int k) { return 0.5f * (b.lo[k] + b.hi[k]); }

// ---------------------------------------------------------------- 2 key
// q = min(2^21 - 1, (int)((c - lo) * (2^21 / (hi - lo)))); 0 on an axis without extent (and where
// the product is not a positive number: an extent that overflows)
YRT_THD uint32_t lbvh_quantize(float c, float lo, float hi) {
  if (!(hi > lo)) return 0u;
  const float f = (c - lo) * (2097152.0f / (hi - lo));
  if (!(f > 0.f)) return 0u;
  if (f >= 2097151.0f) return 2097151u;
  return (uint32_t)(int)f;
}
// bit k of a 21-bit number to bit 3 k
YRT_THD uint64_t lbvh_spread(uint32_t q) {
  uint64_t x = q & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// x, y, z interleaved from bit 62 down; cb: the bounds of all box centres
YRT_THD uint64_t lbvh_key(const LbvhBox& b, const LbvhBox& cb) {
  uint64_t key = 0;
  for (int k = 0; k < 3; ++k)
    key |= lbvh_spread(lbvh_quantize(lbvh_centroid(b, k), cb.lo[k], cb.hi[k])) << (2 - k);
  return key;
}

// ---------------------------------------------------------------- 3 topology
// common prefix of sorted keys i and j; equal keys go on with the prefix of their slots, so the
// keys count as distinct and their order is the slot order
YRT_THD int lbvh_delta(const uint64_t* keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint64_t a = keys[i], b = keys[j];
  if (a == b) return 64 + __builtin_clz((unsigned)(i ^ j));
  return __builtin_clzll(a ^ b);
}
// Node i (0 .. n - 2) covers the sorted slots [first, last] and splits into [first, split] and
// [split + 1, last] (Karras 2012, section 4); it reads the keys only. Node 0 is the root.
YRT_THD void lbvh_range(const uint64_t* keys, int n, int i, int& first, int& last, int& split) {
  const int d = lbvh_delta(keys, n, i, i + 1) > lbvh_delta(keys, n, i, i - 1) ? 1 : -1;
  const int dmin = lbvh_delta(keys, n, i, i - d);
  int lmax = 2;
  while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = lbvh_delta(keys, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  split = i + s * d + (d < 0 ? d : 0);
  first = i < j ? i : j;
  last = i < j ? j : i;
}
// a node is part of the tree when its range is no leaf; the root always is
YRT_THD bool lbvh_is_inner(int i, int first, int last) { return i == 0 || last - first + 1 > YRT_MAX_LEAF; }
// The child references of node i (boxes left alone): the left child is node `split` or a leaf,
// the right child node `split + 1` or a leaf.
YRT_THD void lbvh_node2(int first, int last, int split, LbvhNode2& n) {
  const int lo[2] = {first, split + 1}, hi[2] = {split, last};
  for (int c = 0; c < 2; ++c) {
    const int cnt = hi[c] - lo[c] + 1;
    const bool leaf = cnt <= YRT_MAX_LEAF;
    n.idx[c] = leaf ? lo[c] : (c ? split + 1 : split);
    n.cnt[c] = leaf ? cnt : 0;
  }
}

// ---------------------------------------------------------------- 5 boxes
// Box of child c of a node whose inner children are done (deeper level): the union of the leaf's
// triangles in slot order, or of the inner node's two child boxes.
YRT_THD void lbvh_child_box(const LbvhNode2* nodes, const LbvhBox* primBox, const uint32_t* slotId, int i, int c,
                            LbvhBox& b) {
  lbvh_box_reset(b);
  const int idx = nodes[i].idx[c], cnt = nodes[i].cnt[c];
  if (cnt > 0) {
    for (int t = 0; t < cnt; ++t) lbvh_box_grow(b, primBox[slotId[idx + t]]);
  } else {
    lbvh_box_grow(b, nodes[idx].b[0]);
    lbvh_box_grow(b, nodes[idx].b[1]);
  }
}

// ---------------------------------------------------------------- 6 collapse
// The children of the 4-wide node made from radix-tree node n2: its two children; then, until
// there are four, the inner child of the largest area (ties: the lowest slot) is opened, its left
// child takes the slot and its right child the next free one. Returns the child count (2 .. 4).
YRT_THD int lbvh_collapse(const LbvhNode2* in, int n2, LbvhRef ch[4]) {
  int k = 2;
  for (int j = 0; j < 2; ++j) { ch[j].b = in[n2].b[j]; ch[j].idx = in[n2].idx[j]; ch[j].cnt = in[n2].cnt[j]; }
  while (k < 4) {
    int best = -1;
    float bestArea = -1.f;
    for (int j = 0; j < k; ++j) {
      if (ch[j].cnt != 0) continue;
      const float a = lbvh_box_area(ch[j].b);
      if (a > bestArea) { bestArea = a; best = j; }
    }
    if (best < 0) break;
    const int o = ch[best].idx;
    ch[best].b = in[o].b[0]; ch[best].idx = in[o].idx[0]; ch[best].cnt = in[o].cnt[0];
    ch[k].b = in[o].b[1]; ch[k].idx = in[o].idx[1]; ch[k].cnt = in[o].cnt[1];
    ++k;
  }
  return k;
}
YRT_THD int lbvh_count_inner(const LbvhRef ch[4], int k) {
  int n = 0;
  for (int j = 0; j < k; ++j) n += ch[j].cnt == 0;
  return n;
}
// The 128-B node of children ch[0 .. k): leaves as (slot << 5) | count, the r-th inner child (slot
// order) as node firstInner + r; empty slots the inverted infinite box and -1 (bvh_build.cpp).
// next (k entries at most): the inner children's radix-tree nodes in the same order.
YRT_THD void lbvh_emit(GpuNode& g, const LbvhRef ch[4], int k, int firstInner, int* next) {
  int r = 0;
  for (int j = 0; j < 4; ++j) {
    const bool v = j < k;
    const float L = INFINITY, H = -INFINITY;
    g.lox[j] = v ? ch[j].b.lo[0] : L; g.hix[j] = v ? ch[j].b.hi[0] : H;
    g.loy[j] = v ? ch[j].b.lo[1] : L; g.hiy[j] = v ? ch[j].b.hi[1] : H;
    g.loz[j] = v ? ch[j].b.lo[2] : L; g.hiz[j] = v ? ch[j].b.hi[2] : H;
    g.pad[j] = 0;
    if (!v) {
      g.child[j] = -1;
    } else if (ch[j].cnt > 0) {
      g.child[j] = (ch[j].idx << 5) | ch[j].cnt;
    } else {
      next[r] = ch[j].idx;
      g.child[j] = (firstInner + r) << 5;
      ++r;
    }
  }
}

// ---------------------------------------------------------------- 9 leaf records
// v: 9 floats per triangle id; the .w words as build_bvh writes them (id, flags, 0)
YRT_THD void lbvh_leaf_record(GpuTri& g, const float* v, const uint32_t* flags, uint32_t id) {
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
