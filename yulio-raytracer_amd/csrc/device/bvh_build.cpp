// bvh_build.cpp — host BVH builders for the GPU traversal kernels.
//
// Replaces Embree's rtcCommit SAH build (api/scene_flat.h:72-97).
// build_bvh builds a binned-SAH binary tree (Builder; with YRT_SBVH=1 SplitBuilder, which adds
// spatial splits); build_bvh_morton_host is the serial loop of the scene builder "morton", whose
// binary tree is a radix tree over Morton keys (common/yrt_lbvh.h). Either tree then becomes the
// 4-wide 128-B nodes and 48-B leaf records of common/yrt_gpu_types.h through common/yrt_bvh4.h:
// one collapse rule, one node writer, one leaf-record writer; the builders differ in how they
// number the nodes (here depth-first, morton breadth-first). bvh_limits (bvh_build.h) states what
// the traversal kernels need of every tree: root an inner node, leaves of 1..31 triangles, the
// worst-case traversal stack (3 pushes per 4-wide level) below YRT_STACK_DEPTH (the SAH builders
// force object-median splits below a depth chosen from log2(N)).
#include "bvh_build.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "../common/yrt_lbvh.h"

namespace yrt {

namespace {

#ifndef YRT_SAH_TRAV
#define YRT_SAH_TRAV 1.0f  // SAH cost of a traversal step relative to one triangle test
#endif

// A triangle reference: its box, its id and its centroid, the box's centre. Prim, the default
// builder's, has the centre cached: that builder reads it five times per node and reference
// (centroid bounds, three binning passes, partition) and is measurably slower without. SRef, the
// spatial-split builder's, holds the part of the box inside the node and is copied at every
// split; its centre is taken from the box.
struct Prim {
  Box b;
  float c[3];
  int id;
  float centre(int k) const { return c[k]; }
};
struct SRef {
  Box b;
  int id;
  float centre(int k) const { return b.centre(k); }
};

template <class R>
Box bounds(const R* b, const R* e) {
  Box bb;
  bb.reset();
  for (; b != e; ++b) bb.grow(b->b);
  return bb;
}
template <class R>
Box centroid_bounds(const R* b, const R* e) {
  Box cb;
  cb.reset();
  for (; b != e; ++b) {
    const float c[3] = {b->centre(0), b->centre(1), b->centre(2)};
    cb.growP(c);
  }
  return cb;
}
int widest_axis(const Box& b) {
  int axis = 0;
  for (int k = 1; k < 3; ++k)
    if (b.hi[k] - b.lo[k] > b.hi[axis] - b.lo[axis]) axis = k;
  return axis;
}
bool nonempty(const Box& b) { return b.hi[0] >= b.lo[0] && b.hi[1] >= b.lo[1] && b.hi[2] >= b.lo[2]; }

// Object median of [b, e) along axis; returns the middle.
template <class R>
R* median_split(R* b, R* e, int axis) {
  R* m = b + (e - b) / 2;
  std::nth_element(b, m, e, [axis](const R& x, const R& y) { return x.centre(axis) < y.centre(axis); });
  return m;
}

// ---------------------------------------------------------------- binned SAH
const int NB = 32;
inline int bin_of(float c, float lo, float scale) { return std::min(NB - 1, (int)((c - lo) * scale)); }

struct Split {
  float cost = INFINITY;  // area(L) * count(L) + area(R) * count(R)
  int axis = -1, bin = -1;  // the plane between bin and bin + 1
  Box L, R;                 // the two sides' boxes, where the caller asked for them (side_boxes)
};

// The one bin sweep: the cheapest of the NB - 1 planes of `axis` replaces `best` if it costs less.
// bb: the bins' boxes; enter[k] / leave[k]: the references whose first / last bin is k (an object
// split has every reference in one bin, so both are its count). The left side of plane k holds
// what entered in bins 0 .. k, the right side what leaves in bins k + 1 .. NB - 1. Returns
// whether `best` changed. Most nodes are small, so this sweep is most of a build's time: it keeps
// the right sides' areas, not their boxes; side_boxes gives the winner's.
bool sweep(const Box bb[NB], const int enter[NB], const int leave[NB], int axis, Split& best) {
  float rightArea[NB];
  int rightCnt[NB];
  Box acc;
  acc.reset();
  int ac = 0;
  for (int k = NB - 1; k > 0; --k) {
    acc.grow(bb[k]);
    ac += leave[k];
    rightArea[k] = acc.area();
    rightCnt[k] = ac;
  }
  acc.reset();
  ac = 0;
  for (int k = 0; k < NB - 1; ++k) {
    acc.grow(bb[k]);
    ac += enter[k];
    if (ac == 0 || rightCnt[k + 1] == 0) continue;
    const float cost = acc.area() * ac + rightArea[k + 1] * rightCnt[k + 1];
    if (cost < best.cost) { best.cost = cost; best.axis = axis; best.bin = k; }
  }
  return best.axis == axis;
}
// The boxes left and right of s's plane, grown in the sweep's order (so they are its boxes)
void side_boxes(const Box bb[NB], Split& s) {
  s.L.reset();
  s.R.reset();
  for (int k = 0; k <= s.bin; ++k) s.L.grow(bb[k]);
  for (int k = NB - 1; k > s.bin; --k) s.R.grow(bb[k]);
}

// The best object split of [b, e): references binned by centroid inside the centroid bounds cb.
template <class R>
Split object_split(const R* b, const R* e, const Box& cb, bool boxes) {
  Split best;
  for (int ax = 0; ax < 3; ++ax) {
    const float lo = cb.lo[ax], hi = cb.hi[ax];
    if (!(hi > lo)) continue;
    const float scale = NB / (hi - lo);
    Box bb[NB];
    int cnt[NB] = {0};
    for (int k = 0; k < NB; ++k) bb[k].reset();
    for (const R* x = b; x != e; ++x) {
      const int bin = bin_of(x->centre(ax), lo, scale);
      cnt[bin]++;
      bb[bin].grow(x->b);
    }
    if (sweep(bb, cnt, cnt, ax, best) && boxes) side_boxes(bb, best);
  }
  return best;
}
// Which side of object split s (found inside cb) a reference goes to
struct LeftOf {
  int axis, bin;
  float lo, scale;
  LeftOf(const Split& s, const Box& cb) : axis(s.axis), bin(s.bin), lo(cb.lo[s.axis]), scale(NB / (cb.hi[s.axis] - lo)) {}
  template <class R>
  bool operator()(const R& x) const { return bin_of(x.centre(axis), lo, scale) <= bin; }
};
// n references stay one leaf when that costs no more than the split of cost `cost`
bool leaf_is_cheaper(int n, int maxLeaf, float cost, float parentArea) {
  const float splitCost = YRT_SAH_TRAV + (parentArea > 0.f ? cost / parentArea : (float)n);
  return n <= maxLeaf && (float)n <= splitCost;
}

// ---------------------------------------------------------------- object splits, in place
// The default builder: the references stay in one array, a node is a range of it, and a split
// partitions the range in place (unstably).
struct Builder {
  std::vector<Prim> prims;
  std::vector<Node2> nodes;
  int maxLeaf = YRT_MAX_LEAF;
  int medianDepth = 24;

  // returns split position m (b < m < e)
  int split(int b, int e, int depth, bool& makeLeaf) {
    const int n = e - b;
    Prim* const pb = prims.data() + b;
    Prim* const pe = prims.data() + e;
    makeLeaf = false;
    const Box cb = centroid_bounds(pb, pe);
    const int axis = widest_axis(cb);
    if (!(cb.hi[axis] - cb.lo[axis] > 0.f)) {  // all centroids equal
      if (n <= maxLeaf) { makeLeaf = true; return e; }
      return b + n / 2;
    }
    if (depth >= medianDepth) return (int)(median_split(pb, pe, axis) - prims.data());
    const Split s = object_split(pb, pe, cb, false);
    if (leaf_is_cheaper(n, maxLeaf, s.cost, bounds(pb, pe).area())) { makeLeaf = true; return e; }
    if (s.axis < 0) return b + n / 2;
    const int m = (int)(std::partition(pb, pe, LeftOf(s, cb)) - prims.data());
    return m <= b || m >= e ? b + n / 2 : m;
  }

  // Builds the subtree for [b,e); returns the child reference and its box.
  Ref child(int b, int e, int depth) {
    const Ref leaf{bounds(prims.data() + b, prims.data() + e), b, e - b};
    const int n = e - b;
    if (n <= 2) return leaf;
    bool mkLeaf = false;
    const int m = split(b, e, depth, mkLeaf);
    if (mkLeaf && n <= 31) return leaf;
    return Ref{leaf.b, inner(b, m, e, depth), 0};
  }

  int inner(int b, int m, int e, int depth) {
    const int ni = (int)nodes.size();
    nodes.emplace_back();
    const Ref l = child(b, m, depth + 1);
    const Ref r = child(m, e, depth + 1);
    nodes[ni].set(0, l);
    nodes[ni].set(1, r);
    return ni;
  }
};

// ---------------------------------------------------------------- object and spatial splits
// Spatial-split builder (SBVH, Stich et al. 2009): at each node the binned object split
// (SAH over reference centroids) competes with a binned spatial split, which cuts the node
// box with an axis plane and lets a triangle straddling the plane be referenced from both
// sides with its box clipped to each side. Architectural scenes (long walls, floors, arches)
// have many large triangles whose boxes overlap everything under them; splitting them cuts
// the node visits per ray. The traversal is unaffected: a leaf stores the full triangle, the
// closest hit is the smallest (t, id) over all references, and duplicates only re-test it.
// Spatial splits are tried only where the object split's children overlap by more than
// YRT_SBVH_ALPHA of the root area, and stop once the references exceed (1 + YRT_SBVH_BUDGET) N.
// A node owns its references: a split copies them (stably) into the two children's lists.
#ifndef YRT_SBVH_ALPHA
#define YRT_SBVH_ALPHA 1e-5f
#endif
#ifndef YRT_SBVH_BUDGET
#define YRT_SBVH_BUDGET 0.5f
#endif

// Box of triangle t (9 floats) inside the slab lo <= x[axis] <= hi, padded outward by a
// few ulps on the two other axes (edge/plane intersections round), exact on `axis`.
Box clip_tri(const float* t, int axis, float lo, float hi) {
  Box r;
  r.reset();
  for (int e = 0; e < 3; ++e) {
    const float* p = t + 3 * e;
    const float* q = t + 3 * ((e + 1) % 3);
    const float pa = p[axis], qa = q[axis];
    if (pa >= lo && pa <= hi) r.growP(p);
    const float planes[2] = {lo, hi};
    for (float pl : planes) {
      if ((pa < pl && qa > pl) || (pa > pl && qa < pl)) {
        const double tt = ((double)pl - pa) / ((double)qa - pa);
        float x[3];
        for (int k = 0; k < 3; ++k) x[k] = (float)(p[k] + tt * ((double)q[k] - p[k]));
        x[axis] = pl;
        r.growP(x);
      }
    }
  }
  for (int k = 0; k < 3; ++k) {
    if (k == axis || !(r.hi[k] >= r.lo[k])) continue;
    const float pad = 4.0f * FLT_EPSILON * std::max(fabsf(r.lo[k]), fabsf(r.hi[k]));
    r.lo[k] -= pad;
    r.hi[k] += pad;
  }
  return r;
}

struct SplitBuilder {
  const std::vector<float>& v;
  std::vector<Node2> nodes;
  std::vector<int> leafIds;  // leaf ranges index this (global triangle ids, duplicates allowed)
  int maxLeaf = YRT_MAX_LEAF;
  int medianDepth = 24;
  float minOverlap = 0.f;
  size_t refBudget = 0, numRefs = 0;
  explicit SplitBuilder(const std::vector<float>& verts) : v(verts) {}

  static Box bounds(const std::vector<SRef>& r) { return yrt::bounds(r.data(), r.data() + r.size()); }

  Ref leaf(const std::vector<SRef>& refs, const Box& bb) {
    const Ref r{bb, (int)leafIds.size(), (int)refs.size()};
    for (const SRef& x : refs) leafIds.push_back(x.id);
    return r;
  }

  // Builds the subtree of `refs` (consumed); returns the child reference and its box.
  Ref child(std::vector<SRef>& refs, int depth) {
    const Box bb = bounds(refs);
    const int n = (int)refs.size();
    if (n <= 2) return leaf(refs, bb);
    std::vector<SRef> L, R;
    const bool mkLeaf = split(refs, bb, depth, L, R);
    if (mkLeaf && n <= 31) return leaf(refs, bb);
    if (mkLeaf) median(refs, bb, L, R);
    std::vector<SRef>().swap(refs);
    return Ref{bb, inner(L, R, depth), 0};
  }

  int inner(std::vector<SRef>& L, std::vector<SRef>& R, int depth) {
    const int ni = (int)nodes.size();
    nodes.emplace_back();
    const Ref l = child(L, depth + 1);
    const Ref r = child(R, depth + 1);
    nodes[ni].set(0, l);
    nodes[ni].set(1, r);
    return ni;
  }

  // Object median along the widest axis of bb
  void median(std::vector<SRef>& refs, const Box& bb, std::vector<SRef>& L, std::vector<SRef>& R) {
    SRef* const b = refs.data();
    SRef* const e = b + refs.size();
    SRef* const m = median_split(b, e, widest_axis(bb));
    L.assign(b, m);
    R.assign(m, e);
  }

  // The best spatial split of `refs`: a reference enters the bin of its box's low end and leaves
  // that of its high end; in between, each bin gets the triangle clipped to the bin's slab.
  Split spatial_split(const std::vector<SRef>& refs, const Box& nodeBox) const {
    Split best;
    for (int ax = 0; ax < 3; ++ax) {
      const float lo = nodeBox.lo[ax], hi = nodeBox.hi[ax];
      if (!(hi > lo)) continue;
      const float w = (hi - lo) / NB;
      Box bb[NB];
      int enter[NB] = {0}, leave[NB] = {0};
      for (int k = 0; k < NB; ++k) bb[k].reset();
      for (const SRef& x : refs) {
        const int b0 = std::max(0, std::min(NB - 1, (int)((x.b.lo[ax] - lo) / w)));
        const int b1 = std::max(b0, std::min(NB - 1, (int)((x.b.hi[ax] - lo) / w)));
        enter[b0]++;
        leave[b1]++;
        if (b0 == b1) {
          bb[b0].grow(x.b);
          continue;
        }
        const float* t = &v[(size_t)x.id * 9];
        for (int k = b0; k <= b1; ++k) {
          const float s0 = k == b0 ? x.b.lo[ax] : lo + k * w;
          const float s1 = k == b1 ? x.b.hi[ax] : lo + (k + 1) * w;
          const Box cbx = intersect(clip_tri(t, ax, s0, s1), x.b);
          if (nonempty(cbx)) bb[k].grow(cbx);
        }
      }
      sweep(bb, enter, leave, ax, best);
    }
    return best;
  }

  // Chooses leaf / object split / spatial split; fills L, R unless a leaf is chosen.
  bool split(std::vector<SRef>& refs, const Box& nodeBox, int depth, std::vector<SRef>& L, std::vector<SRef>& R) {
    const int n = (int)refs.size();
    const Box cb = centroid_bounds(refs.data(), refs.data() + n);
    if (depth >= medianDepth) {
      median(refs, cb, L, R);
      return false;
    }
    const Split obj = object_split(refs.data(), refs.data() + n, cb, true);
    // spatial split, where the object split's children overlap
    Split sp;
    const float overlap = obj.axis >= 0 ? intersect(obj.L, obj.R).area() : INFINITY;
    if (numRefs < refBudget && overlap > minOverlap) sp = spatial_split(refs, nodeBox);
    if (leaf_is_cheaper(n, maxLeaf, std::min(obj.cost, sp.cost), nodeBox.area())) return true;
    if (obj.axis < 0 && sp.axis < 0) return true;  // caller falls back to a median split
    if (sp.axis >= 0 && sp.cost < obj.cost) {
      const float lo = nodeBox.lo[sp.axis], w = (nodeBox.hi[sp.axis] - lo) / NB;
      const float plane = lo + (sp.bin + 1) * w;
      for (const SRef& x : refs) {
        if (x.b.hi[sp.axis] <= plane) { L.push_back(x); continue; }
        if (x.b.lo[sp.axis] >= plane) { R.push_back(x); continue; }
        const float* t = &v[(size_t)x.id * 9];
        const Box bl = intersect(clip_tri(t, sp.axis, x.b.lo[sp.axis], plane), x.b);
        const Box br = intersect(clip_tri(t, sp.axis, plane, x.b.hi[sp.axis]), x.b);
        const bool okL = nonempty(bl), okR = nonempty(br);
        if (okL) L.push_back(SRef{bl, x.id});
        if (okR) R.push_back(SRef{br, x.id});
        if (!okL && !okR) (x.centre(sp.axis) < plane ? L : R).push_back(x);  // degenerate clip: keep whole
        if (okL && okR) numRefs++;
      }
      if (!L.empty() && !R.empty()) return false;
      // degenerate (everything on one side): fall back to the object split
      refs.clear();
      for (auto* side : {&L, &R})
        for (const SRef& x : *side) refs.push_back(x);
      L.clear();
      R.clear();
      if (obj.axis < 0) return true;
    }
    const LeftOf left(obj, cb);
    for (const SRef& x : refs) (left(x) ? L : R).push_back(x);
    if (L.empty() || R.empty()) {
      L.clear();
      R.clear();
      return true;
    }
    return false;
  }
};

// ---------------------------------------------------------------- binary tree -> 4-wide nodes
// Depth-first pre-order: a node takes its index before its children are collapsed, so a subtree
// is one run of nodes. maxStack: the worst-case traversal stack, the largest sum over a root
// path of (children - 1).
struct Collapser {
  const std::vector<Node2>& in;
  std::vector<GpuNode> out;
  int maxStack = 0;
  explicit Collapser(const std::vector<Node2>& n) : in(n) {}

  // Emits the 4-wide node for binary inner node `n2`; returns its index.
  int collapse(int n2, int stackAbove) {
    Ref ch[4];
    const int k = collapse4(in.data(), n2, ch);
    const int ni = (int)out.size();
    out.emplace_back();
    const int stackHere = stackAbove + (k - 1);
    maxStack = std::max(maxStack, stackHere);
    int node[4] = {0, 0, 0, 0};
    for (int j = 0; j < k; ++j)
      if (ch[j].cnt == 0) node[j] = collapse(ch[j].idx, stackHere);
    write_node4(out[ni], ch, k, node);
    return ni;
  }
};

}  // namespace

void build_bvh(const std::vector<float>& v /* 9 floats per triangle */, const std::vector<uint32_t>& flags,
               int stackDepth, BvhResult& out, const std::vector<float>* v1) {
  const int N = (int)(v.size() / 9);
  out.nodes.clear();
  out.tris.clear();
  out.order.clear();
  if (N == 0) return;
  // A BVH2 path of depth D collapses to about D/2 four-wide levels of <= 3 pushes each.
  const int levels = (int)ceil(log2(std::max(1.0, N / 16.0)));
  const int medianDepth = std::max(0, std::min(28, (2 * stackDepth) / 3 - 2 - levels));
  std::vector<Node2> nodes2;
  std::vector<int> leafIds;  // leaf slot -> global triangle id
  // spatial splits are opt-in (YRT_SBVH=1): on the measured scenes (C2-C4 stand-ins) they cut
  // node visits by < 1 % for 2-5x the build time
  const char* env = getenv("YRT_SBVH");
  const bool spatial = env && atoi(env) != 0 && !v1;  // spatial splits clip static triangles only
  // a triangle's box bounds both ends of the frame time
  auto tri_box = [&](int i) {
    Box b;
    b.reset();
    for (int k = 0; k < 3; ++k) b.growP(&v[(size_t)i * 9 + 3 * k]);
    if (v1)
      for (int k = 0; k < 3; ++k) b.growP(&(*v1)[(size_t)i * 9 + 3 * k]);
    return b;
  };
  if (N == 1) {  // the root has to be an inner node: the triangle twice
    const Ref leaf{tri_box(0), 0, 1};
    nodes2.emplace_back();
    nodes2[0].set(0, leaf);
    nodes2[0].set(1, leaf);
    leafIds.push_back(0);
  } else if (spatial) {
    SplitBuilder B(v);
    B.medianDepth = medianDepth;
    std::vector<SRef> refs(N);
    for (int i = 0; i < N; ++i) refs[i] = SRef{tri_box(i), i};
    const Box root = SplitBuilder::bounds(refs);
    B.minOverlap = YRT_SBVH_ALPHA * root.area();
    B.numRefs = (size_t)N;
    B.refBudget = (size_t)(N * (1.0 + YRT_SBVH_BUDGET));
    std::vector<SRef> L, R;
    bool leaf = B.split(refs, root, 0, L, R);
    if (leaf) B.median(refs, root, L, R);
    std::vector<SRef>().swap(refs);
    B.inner(L, R, 0);
    nodes2 = std::move(B.nodes);
    leafIds = std::move(B.leafIds);
  } else {
    Builder B;
    B.medianDepth = medianDepth;
    B.prims.resize(N);
    for (int i = 0; i < N; ++i) {
      Prim& p = B.prims[i];
      p.b = tri_box(i);
      for (int k = 0; k < 3; ++k) p.c[k] = p.b.centre(k);
      p.id = i;
    }
    bool leaf = false;
    int m = B.split(0, N, 0, leaf);
    if (leaf || m <= 0 || m >= N) m = N / 2;
    B.inner(0, m, N, 0);
    nodes2 = std::move(B.nodes);
    leafIds.resize(N);
    for (int i = 0; i < N; ++i) leafIds[i] = B.prims[i].id;
  }
  Collapser C(nodes2);
  C.collapse(0, 0);
  out.maxDepth = C.maxStack;
  const char* why = nullptr;
  if (bvh_limits(C.out.size(), leafIds.size(), C.maxStack, stackDepth, &why)) throw std::runtime_error(why);
  out.nodes = std::move(C.out);
  const size_t S = leafIds.size();
  out.order = leafIds;
  out.tris.resize(S);
  for (size_t i = 0; i < S; ++i) write_leaf_record(out.tris[i], v.data(), flags.data(), (uint32_t)leafIds[i]);
}

// ---------------------------------------------------------------- scene builder "morton", host loop
// The steps of common/yrt_lbvh.h and yrt_bvh4.h over every element in turn, in the order in which
// kernels/bvh_build.hip launches them; the "host" device builds with this loop (builder 2), and
// the GPU tests require the kernels to give its bytes.
int build_bvh_morton_host(const std::vector<float>& v, const std::vector<uint32_t>& flags, int stackDepth,
                          BvhResult& out, const std::vector<float>* v1) {
  const size_t N64 = v.size() / 9;
  if (N64 < 2) return FALLBACK_FEW_TRIANGLES;
  if (BuildFallback f = bvh_limits(0, N64, 0, stackDepth)) return f;
  const int N = (int)N64;
  // 1 boxes, centroid bounds
  std::vector<Box> box(N);
  Box cb;
  cb.reset();
  bool finite = true;
  for (int i = 0; i < N; ++i) {
    finite = lbvh_prim_box(&v[(size_t)i * 9], v1 ? &(*v1)[(size_t)i * 9] : nullptr, box[i]) && finite;
    const float c[3] = {box[i].centre(0), box[i].centre(1), box[i].centre(2)};
    cb.growP(c);
  }
  if (!finite) return FALLBACK_NON_FINITE;
  // 2 keys, stable sort
  std::vector<uint64_t> key(N), keys(N);
  std::vector<uint32_t> slotId(N);
  for (int i = 0; i < N; ++i) { key[i] = lbvh_key(box[i], cb); slotId[i] = (uint32_t)i; }
  std::stable_sort(slotId.begin(), slotId.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  for (int i = 0; i < N; ++i) keys[i] = key[slotId[i]];
  // 3, 4 hierarchy, leaves, levels
  std::vector<Node2> nodes2(N - 1);
  std::vector<int> parent(N - 1, -1);
  std::vector<char> inner(N - 1, 0);
  for (int i = 0; i < N - 1; ++i) {
    int first, last, split;
    lbvh_range(keys.data(), N, i, first, last, split);
    if (!lbvh_is_inner(i, first, last)) continue;
    inner[i] = 1;
    lbvh_node2(first, last, split, nodes2[i]);
    for (int c = 0; c < 2; ++c)
      if (nodes2[i].cnt[c] == 0) parent[nodes2[i].idx[c]] = i;
  }
  std::vector<std::vector<int>> levels;
  for (int i = 0; i < N - 1; ++i) {
    if (!inner[i]) continue;
    int d = 0;
    for (int p = parent[i]; p >= 0; p = parent[p]) ++d;
    if (d >= YRT_LBVH_MAX_LEVELS) return FALLBACK_STACK;
    if ((int)levels.size() <= d) levels.resize(d + 1);
    levels[d].push_back(i);
  }
  // 5 boxes, deepest level first
  for (int d = (int)levels.size() - 1; d >= 0; --d)
    for (int i : levels[d])
      for (int c = 0; c < 2; ++c) {
        Box b;
        lbvh_child_box(nodes2.data(), box.data(), slotId.data(), i, c, b);
        nodes2[i].b[c] = b;
      }
  // 6 - 8 collapse, one 4-wide level at a time; numbered by an exclusive scan over the level
  std::vector<GpuNode> nodes;
  std::vector<int> frontier = {0}, stackAbove = {0}, next, nextStack, off;
  int maxStack = 0;
  for (int level = 0; !frontier.empty(); ++level) {
    if (level >= YRT_LBVH_MAX_LEVELS) return FALLBACK_STACK;
    const size_t base = nodes.size(), cnt = frontier.size();
    if (BuildFallback f = bvh_limits(base + cnt, N64, 0, stackDepth)) return f;
    off.assign(cnt, 0);
    int total = 0;
    Ref ch[4];
    for (size_t f = 0; f < cnt; ++f) {
      off[f] = total;
      total += lbvh_count_inner(ch, collapse4(nodes2.data(), frontier[f], ch));
    }
    nodes.resize(base + cnt);
    next.assign(total, 0);
    nextStack.assign(total, 0);
    for (size_t f = 0; f < cnt; ++f) {
      const int k = collapse4(nodes2.data(), frontier[f], ch);
      const int stackHere = stackAbove[f] + (k - 1);
      maxStack = std::max(maxStack, stackHere);
      int node[4], nx[4];
      const int ni = lbvh_number(ch, k, (int)(base + cnt) + off[f], node, nx);
      write_node4(nodes[base + f], ch, k, node);
      for (int r = 0; r < ni; ++r) { next[off[f] + r] = nx[r]; nextStack[off[f] + r] = stackHere; }
    }
    frontier.swap(next);
    stackAbove.swap(nextStack);
  }
  if (BuildFallback f = bvh_limits(nodes.size(), N64, maxStack, stackDepth)) return f;
  // 9 leaf records: sorted order is leaf order
  out.maxDepth = maxStack;
  out.nodes = std::move(nodes);
  out.order.assign(slotId.begin(), slotId.end());
  out.tris.resize(N);
  for (int i = 0; i < N; ++i) write_leaf_record(out.tris[i], v.data(), flags.data(), slotId[i]);
  return FALLBACK_NONE;
}

double bvh_sah_cost(const std::vector<GpuNode>& nodes) {
  if (nodes.empty()) return 0;
  auto area = [](const GpuNode& n, int j) {
    const double dx = (double)n.hix[j] - n.lox[j], dy = (double)n.hiy[j] - n.loy[j], dz = (double)n.hiz[j] - n.loz[j];
    return dx >= 0 && dy >= 0 && dz >= 0 ? 2.0 * (dx * dy + dy * dz + dz * dx) : 0.0;
  };
  Box root;
  root.reset();
  for (int j = 0; j < 4; ++j) {
    if (nodes[0].child[j] == -1) continue;
    const GpuNode& n = nodes[0];
    const Box b = {{n.lox[j], n.loy[j], n.loz[j]}, {n.hix[j], n.hiy[j], n.hiz[j]}};
    root.grow(b);
  }
  const double dx = (double)root.hi[0] - root.lo[0], dy = (double)root.hi[1] - root.lo[1], dz = (double)root.hi[2] - root.lo[2];
  const double rootArea = 2.0 * (dx * dy + dy * dz + dz * dx);
  if (!(rootArea > 0) || !std::isfinite(rootArea)) return 0;
  double cost = 0;
  for (const GpuNode& n : nodes)
    for (int j = 0; j < 4; ++j) {
      const int c = n.child[j];
      if (c == -1) continue;
      cost += area(n, j) * ((c & 31) ? (double)(c & 31) : (double)YRT_SAH_TRAV);
    }
  return cost / rootArea;
}

}  // namespace yrt
