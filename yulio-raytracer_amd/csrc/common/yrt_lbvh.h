// yrt_lbvh.h — the Morton-specific per-element steps of the scene builder "morton" (LBVH, Karras
// 2012, collapsed to 4-wide nodes), written once: the kernels of kernels/k_bvh_build.h and the
// serial host loop of device/bvh_build.cpp call the same functions, so both give the same bytes.
// What the builder shares with the host SAH builders (the box, the binary node, the collapse rule,
// the node and leaf-record writers) is yrt_bvh4.h's.
//
//   1 lbvh_prim_box       vertex bounds of a triangle (both ends of the frame time), finiteness
//   2 lbvh_key            63-bit Morton code of the box centre inside the centroid bounds
//   3 lbvh_range          node i of the N - 1 radix-tree nodes: its key range and split
//     lbvh_node2          the node's two child references; a range of <= YRT_MAX_LEAF keys is a leaf
//   5 lbvh_child_box      a child's box, bottom-up: the exact union of its triangles' / its node's boxes
//   6 collapse4           the children of one 4-wide node (yrt_bvh4.h)
//   7 lbvh_number         breadth-first numbering: a level's inner children follow the level
//     write_node4         the 128-B node (yrt_bvh4.h)
//   9 write_leaf_record   the leaf record of a sorted slot (yrt_bvh4.h)
#pragma once

#include <math.h>
#include <stdint.h>

#include "yrt_bvh4.h"

#ifndef YRT_MAX_LEAF
#define YRT_MAX_LEAF 8
#endif
// levels of the radix tree the build can hold: 63 key bits + 32 index bits (equal keys) bound it
#define YRT_LBVH_MAX_LEVELS 128

namespace yrt {

// ---------------------------------------------------------------- 1 primitive box
// v, v1: the triangle's 9 floats at time 0 and (moving scenes, else null) time 1. Returns false
// when a coordinate or the box centre is not finite.
YRT_THD bool lbvh_prim_box(const float* v, const float* v1, Box& b) {
  b.reset();
  bool ok = true;
  for (int s = 0; s < 2; ++s) {
    const float* p = s ? v1 : v;
    if (!p) continue;
    for (int j = 0; j < 9; ++j) ok = ok && (p[j] - p[j] == 0.f);
    for (int j = 0; j < 3; ++j) b.growP(p + 3 * j);
  }
  for (int k = 0; k < 3; ++k) {
    const float c = b.centre(k);
    ok = ok && (c - c == 0.f);
  }
  return ok;
}

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
YRT_THD uint64_t lbvh_key(const Box& b, const Box& cb) {
  uint64_t key = 0;
  for (int k = 0; k < 3; ++k)
    key |= lbvh_spread(lbvh_quantize(b.centre(k), cb.lo[k], cb.hi[k])) << (2 - k);
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
YRT_THD void lbvh_node2(int first, int last, int split, Node2& n) {
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
YRT_THD void lbvh_child_box(const Node2* nodes, const Box* primBox, const uint32_t* slotId, int i, int c,
                            Box& b) {
  b.reset();
  const int idx = nodes[i].idx[c], cnt = nodes[i].cnt[c];
  if (cnt > 0) {
    for (int t = 0; t < cnt; ++t) b.grow(primBox[slotId[idx + t]]);
  } else {
    b.grow(nodes[idx].b[0]);
    b.grow(nodes[idx].b[1]);
  }
}

// ---------------------------------------------------------------- 7 numbering
YRT_THD int lbvh_count_inner(const Ref ch[4], int k) {
  int n = 0;
  for (int j = 0; j < k; ++j) n += ch[j].cnt == 0;
  return n;
}
// Breadth-first: the r-th inner child (slot order) of ch[0 .. k) is node firstInner + r, and
// next[r] its radix-tree node. Returns the number of inner children.
YRT_THD int lbvh_number(const Ref ch[4], int k, int firstInner, int node[4], int next[4]) {
  int r = 0;
  for (int j = 0; j < k; ++j)
    if (ch[j].cnt == 0) { node[j] = firstInner + r; next[r++] = ch[j].idx; }
  return r;
}

}  // namespace yrt
