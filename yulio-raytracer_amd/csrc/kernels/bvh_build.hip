// bvh_build.hip — the scene builder "morton" on the GPU: the launches of k_bvh_build.h in the
// order of the host loop (device/bvh_build.cpp build_bvh_morton_host), rocPRIM's radix sort and
// exclusive scan between them. A translation unit of its own: kernels/pathtrace.hip and its code
// object are not touched.
//
//   prims -> keys -> sort (key, id) -> hierarchy -> depth -> sort (depth, node) -> level starts
//   [read back: flags, levels] -> boxes per level, deepest first -> per 4-wide level: count,
//   scan, emit [read back: the next level's size] -> leaf records -> download
//
// The host reads a level's size back before it launches the next level, so every grid and every
// offset is a host-checked number; a tree has a few dozen levels of either kind.
#include <cstddef>
#include <cstring>  // before rocprim.hpp: its headers use memcpy unqualified

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../device/bvh_build.h"
#include "k_bvh_build.h"

namespace yrt {

namespace {

#define LBVH_CHECK(x)                                                                             \
  do {                                                                                            \
    hipError_t _e = (x);                                                                          \
    if (_e != hipSuccess)                                                                         \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #x);    \
  } while (0)

struct Buf {
  void* p = nullptr;
  Buf() {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t bytes) { LBVH_CHECK(hipMalloc(&p, bytes ? bytes : 16)); }
  template <class T>
  T* as() const { return (T*)p; }
};

// HIP-event time of the stream's work between the synchronisations (timing on)
struct Segments {
  hipStream_t s;
  bool on;
  hipEvent_t a = nullptr, b = nullptr;
  double ms = 0;
  Segments(hipStream_t st, bool timing) : s(st), on(timing) {
    if (!on) return;
    LBVH_CHECK(hipEventCreate(&a));
    LBVH_CHECK(hipEventCreate(&b));
    LBVH_CHECK(hipEventRecord(a, s));
  }
  ~Segments() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void sync() {
    if (on) LBVH_CHECK(hipEventRecord(b, s));
    LBVH_CHECK(hipStreamSynchronize(s));
    if (!on) return;
    float t = 0;
    LBVH_CHECK(hipEventElapsedTime(&t, a, b));
    ms += t;
    LBVH_CHECK(hipEventRecord(a, s));
  }
};

// the collapse reads maxStack and nextCount back in one copy
static_assert(offsetof(LbvhState, nextCount) == offsetof(LbvhState, maxStack) + sizeof(int), "LbvhState layout");

inline unsigned blocks(size_t n) { return (unsigned)((n + YRT_LBVH_BLOCK - 1) / YRT_LBVH_BLOCK); }

}  // namespace

int build_bvh_morton_gpu(const std::vector<float>& v, const std::vector<uint32_t>& flags, int stackDepth,
                         BvhResult& out, const std::vector<float>* v1, void* stream, bool timing, double* msKernels) {
  hipStream_t s = (hipStream_t)stream;
  if (msKernels) *msKernels = 0;
  const size_t N64 = v.size() / 9;
  if (N64 < 2) return FALLBACK_FEW_TRIANGLES;
  if (BuildFallback f = bvh_limits(0, N64, 0, stackDepth)) return f;
  if (flags.size() < N64 || (v1 && v1->size() < N64 * 9)) return FALLBACK_SIZE;
  const int N = (int)N64, M = N - 1;  // M radix-tree nodes

  // temporaries, all sized from N before the first launch
  Buf dV, dV1, dFlags, dBox, dState, dKeyA, dKeyB, dIdA, dSlot, dNodes2, dParent, dInner, dDepthA, dDepthB, dNodeA,
      dLevelNodes, dTris, dTemp;
  size_t tmpSort = 0, tmpSort2 = 0, tmpScan = 0;
  LBVH_CHECK(rocprim::radix_sort_pairs(nullptr, tmpSort, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                       (uint32_t*)nullptr, (size_t)N, 0u, 63u, s));
  LBVH_CHECK(rocprim::radix_sort_pairs(nullptr, tmpSort2, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                       (uint32_t*)nullptr, (size_t)M, 0u, 8u, s));
  LBVH_CHECK(rocprim::exclusive_scan(nullptr, tmpScan, (int*)nullptr, (int*)nullptr, 0, (size_t)M,
                                     rocprim::plus<int>(), s));
  const size_t tmpBytes = std::max(tmpSort, std::max(tmpSort2, tmpScan));
  dV.alloc(N64 * 9 * sizeof(float));
  if (v1) dV1.alloc(N64 * 9 * sizeof(float));
  dFlags.alloc(N64 * sizeof(uint32_t));
  dBox.alloc(N64 * sizeof(Box));
  dState.alloc(sizeof(LbvhState));
  dKeyA.alloc(N64 * 8);
  dKeyB.alloc(N64 * 8);
  dIdA.alloc(N64 * 4);
  dSlot.alloc(N64 * 4);
  dNodes2.alloc((size_t)M * sizeof(Node2));
  dParent.alloc((size_t)M * 4);
  dInner.alloc((size_t)M * 4);
  dDepthA.alloc((size_t)M * 4);
  dDepthB.alloc((size_t)M * 4);
  dNodeA.alloc((size_t)M * 4);
  dLevelNodes.alloc((size_t)M * 4);
  dTris.alloc(N64 * sizeof(GpuTri));
  dTemp.alloc(tmpBytes);

  LbvhState h;
  memset(&h, 0, sizeof(h));
  for (int k = 0; k < 3; ++k) { h.cbLo[k] = ~0u; h.cbHi[k] = 0u; }
  LBVH_CHECK(hipMemcpyAsync(dV.p, v.data(), N64 * 9 * sizeof(float), hipMemcpyHostToDevice, s));
  if (v1) LBVH_CHECK(hipMemcpyAsync(dV1.p, v1->data(), N64 * 9 * sizeof(float), hipMemcpyHostToDevice, s));
  LBVH_CHECK(hipMemcpyAsync(dFlags.p, flags.data(), N64 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  LBVH_CHECK(hipMemcpyAsync(dState.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
  LBVH_CHECK(hipMemsetAsync(dParent.p, 0xff, (size_t)M * 4, s));
  LBVH_CHECK(hipStreamSynchronize(s));  // the uploads are not kernel time

  Segments seg(s, timing);
  LbvhState* st = dState.as<LbvhState>();
  k_lbvh_prims<<<blocks(N), YRT_LBVH_BLOCK, 0, s>>>(dV.as<float>(), v1 ? dV1.as<float>() : nullptr, N,
                                                    dBox.as<Box>(), st);
  k_lbvh_keys<<<blocks(N), YRT_LBVH_BLOCK, 0, s>>>(dBox.as<Box>(), st, N, dKeyA.as<uint64_t>(),
                                                   dIdA.as<uint32_t>());
  size_t tb = tmpBytes;
  LBVH_CHECK(rocprim::radix_sort_pairs(dTemp.p, tb, dKeyA.as<uint64_t>(), dKeyB.as<uint64_t>(), dIdA.as<uint32_t>(),
                                       dSlot.as<uint32_t>(), (size_t)N, 0u, 63u, s));
  k_lbvh_hierarchy<<<blocks(M), YRT_LBVH_BLOCK, 0, s>>>(dKeyB.as<uint64_t>(), N, dNodes2.as<Node2>(),
                                                        dParent.as<int>(), dInner.as<int>());
  k_lbvh_depth<<<blocks(M), YRT_LBVH_BLOCK, 0, s>>>(dParent.as<int>(), dInner.as<int>(), M, dDepthA.as<uint32_t>(),
                                                    dNodeA.as<uint32_t>(), st);
  tb = tmpBytes;
  LBVH_CHECK(rocprim::radix_sort_pairs(dTemp.p, tb, dDepthA.as<uint32_t>(), dDepthB.as<uint32_t>(),
                                       dNodeA.as<uint32_t>(), dLevelNodes.as<uint32_t>(), (size_t)M, 0u, 8u, s));
  k_lbvh_level_starts<<<blocks(M), YRT_LBVH_BLOCK, 0, s>>>(dDepthB.as<uint32_t>(), M, st);
  LBVH_CHECK(hipGetLastError());
  LBVH_CHECK(hipMemcpyAsync(&h, dState.p, sizeof(h), hipMemcpyDeviceToHost, s));
  seg.sync();
  if (h.nonFinite) return FALLBACK_NON_FINITE;
  if (h.tooDeep || h.numLevels < 1 || h.numLevels > YRT_LBVH_MAX_LEVELS) return FALLBACK_STACK;
  const int live = h.levelStart[h.numLevels];  // inner radix-tree nodes: the 4-wide nodes are a subset
  if (h.levelStart[0] != 0 || live < 1 || live > M) throw std::runtime_error("morton build: level table out of range");
  for (int d = 0; d < h.numLevels; ++d)
    if (h.levelStart[d + 1] <= h.levelStart[d]) throw std::runtime_error("morton build: level table not increasing");

  for (int d = h.numLevels - 1; d >= 0; --d) {
    const int cnt = h.levelStart[d + 1] - h.levelStart[d];
    k_lbvh_boxes<<<blocks(cnt), YRT_LBVH_BLOCK, 0, s>>>(dNodes2.as<Node2>(), dBox.as<Box>(),
                                                        dSlot.as<uint32_t>(),
                                                        dLevelNodes.as<uint32_t>() + h.levelStart[d], cnt);
  }

  Buf dOut, dFrontA, dFrontB, dStackA, dStackB, dNumInner, dOff;
  dOut.alloc((size_t)live * sizeof(GpuNode));
  for (Buf* b : {&dFrontA, &dFrontB, &dStackA, &dStackB, &dNumInner, &dOff}) b->alloc((size_t)live * 4);
  LBVH_CHECK(hipMemsetAsync(dFrontA.p, 0, 4, s));  // the root: radix-tree node 0, nothing on the stack above it
  LBVH_CHECK(hipMemsetAsync(dStackA.p, 0, 4, s));
  int base = 0, cnt = 1;
  int *front = dFrontA.as<int>(), *next = dFrontB.as<int>(), *stk = dStackA.as<int>(), *nstk = dStackB.as<int>();
  for (int level = 0; cnt > 0; ++level) {
    if (level >= YRT_LBVH_MAX_LEVELS) return FALLBACK_STACK;
    if (BuildFallback f = bvh_limits((size_t)base + (size_t)cnt, N64, 0, stackDepth)) return f;
    if (base + cnt > live) throw std::runtime_error("morton build: more 4-wide nodes than radix-tree nodes");
    k_lbvh_count<<<blocks(cnt), YRT_LBVH_BLOCK, 0, s>>>(dNodes2.as<Node2>(), front, cnt, dNumInner.as<int>());
    tb = tmpBytes;
    LBVH_CHECK(rocprim::exclusive_scan(dTemp.p, tb, dNumInner.as<int>(), dOff.as<int>(), 0, (size_t)cnt,
                                       rocprim::plus<int>(), s));
    k_lbvh_emit<<<blocks(cnt), YRT_LBVH_BLOCK, 0, s>>>(dNodes2.as<Node2>(), front, stk, dOff.as<int>(), cnt, base,
                                                       dOut.as<GpuNode>(), next, nstk, live, st);
    LBVH_CHECK(hipGetLastError());
    LBVH_CHECK(hipMemcpyAsync(&h.maxStack, &st->maxStack, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    seg.sync();
    if (h.nextCount < 0 || base + cnt + h.nextCount > live)
      throw std::runtime_error("morton build: a level larger than the tree");
    base += cnt;
    cnt = h.nextCount;
    std::swap(front, next);
    std::swap(stk, nstk);
  }
  if (BuildFallback f = bvh_limits((size_t)base, N64, h.maxStack, stackDepth)) return f;

  k_lbvh_leaves<<<blocks(N), YRT_LBVH_BLOCK, 0, s>>>(dV.as<float>(), dFlags.as<uint32_t>(), dSlot.as<uint32_t>(), N,
                                                     dTris.as<GpuTri>());
  LBVH_CHECK(hipGetLastError());
  seg.sync();
  if (msKernels) *msKernels = seg.ms;

  out.maxDepth = h.maxStack;
  out.nodes.resize(base);
  out.tris.resize(N);
  out.order.resize(N);
  static_assert(sizeof(int) == sizeof(uint32_t), "order holds the sorted ids");
  LBVH_CHECK(hipMemcpyAsync(out.nodes.data(), dOut.p, (size_t)base * sizeof(GpuNode), hipMemcpyDeviceToHost, s));
  LBVH_CHECK(hipMemcpyAsync(out.tris.data(), dTris.p, N64 * sizeof(GpuTri), hipMemcpyDeviceToHost, s));
  LBVH_CHECK(hipMemcpyAsync(out.order.data(), dSlot.p, N64 * 4, hipMemcpyDeviceToHost, s));
  LBVH_CHECK(hipStreamSynchronize(s));
  return FALLBACK_NONE;
}

}  // namespace yrt
