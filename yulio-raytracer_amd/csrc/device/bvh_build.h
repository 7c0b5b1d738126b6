// bvh_build.h — the 4-wide BVH builders (see bvh_build.cpp, kernels/bvh_build.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../common/yrt_gpu_types.h"

namespace yrt {

struct BvhResult {
  std::vector<GpuNode> nodes;
  std::vector<GpuTri> tris;   // leaf order
  std::vector<int> order;     // leaf slot -> global triangle id
  int maxDepth = 0;           // worst-case traversal stack entries (scene info 'bvhDepth')
};

// v: 9 floats (v0,v1,v2) per global triangle id; flags: per-triangle GpuTri flags (bit0 cull)
// v1 (optional): the triangles' vertices at the end of the frame time (moving geometry); the
// boxes then bound both (trianglemesh_full.cpp:152-166), the leaf records hold the t = 0 triangle
void build_bvh(const std::vector<float>& v, const std::vector<uint32_t>& flags, int stackDepth, BvhResult& out,
               const std::vector<float>* v1 = nullptr);

// ---------------------------------------------------------------- scene builder "morton"
// An LBVH (63-bit Morton keys, Karras 2012) collapsed to the same 4-wide nodes; the steps are in
// common/yrt_lbvh.h and common/yrt_bvh4.h. The result depends on the triangles alone: the serial
// host loop and the kernels (kernels/bvh_build.hip) give the same bytes on every run. Both take
// build_bvh's arguments and return 0 with `out` filled, or the reason why the caller has to use build_bvh:
enum BuildFallback {
  FALLBACK_NONE = 0,
  FALLBACK_FEW_TRIANGLES = 1,  // fewer than 2
  FALLBACK_NON_FINITE = 2,     // a vertex (or a box centre) is not finite
  FALLBACK_STACK = 3,          // the worst-case traversal stack exceeds stackDepth - 1
  FALLBACK_SIZE = 4            // node / reference limits (bvh_limits)
};
// What every tree has to meet, whoever built it: the worst-case traversal stack fits the kernels'
// (stackDepth - 1 entries), and a child reference packs (index << 5) | count into an int while
// the traversal addresses a node by a 32-bit byte offset, (index << 6) for the quantized nodes
// (kernels/yrt_traverse.h qnode_load) and (index << 7) for the float ones: 2^25 nodes, 2^26 leaf
// triangle references. Returns FALLBACK_NONE or the limit that is exceeded (why: in words).
inline BuildFallback bvh_limits(size_t numNodes, size_t numRefs, int maxStack, int stackDepth,
                                const char** why = nullptr) {
  const char* w = nullptr;
  BuildFallback f = FALLBACK_NONE;
  if (maxStack > stackDepth - 1) {
    f = FALLBACK_STACK;
    w = "BVH traversal stack bound exceeds YRT_STACK_DEPTH";
  } else if (numNodes >= (size_t(1) << 25)) {
    f = FALLBACK_SIZE;
    w = "BVH exceeds 2^25 nodes (32-bit node byte offsets)";
  } else if (numRefs >= (size_t(1) << 26)) {
    f = FALLBACK_SIZE;
    w = "BVH exceeds 2^26 leaf triangle references (child reference packing)";
  }
  if (why) *why = w;
  return f;
}
enum BuilderKind { BUILDER_SAH = 0, BUILDER_MORTON_GPU = 1, BUILDER_MORTON_HOST = 2 };
int build_bvh_morton_host(const std::vector<float>& v, const std::vector<uint32_t>& flags, int stackDepth,
                          BvhResult& out, const std::vector<float>* v1 = nullptr);
// On the current HIP device, in `stream` (a hipStream_t); returns after the tree is downloaded.
// msKernels (timing only): summed HIP-event time of the build's kernels.
int build_bvh_morton_gpu(const std::vector<float>& v, const std::vector<uint32_t>& flags, int stackDepth,
                         BvhResult& out, const std::vector<float>* v1, void* stream, bool timing, double* msKernels);

// What yrtGetSceneBuildInfo reports of a commit's BVH step
struct BuildInfo {
  int builder = BUILDER_SAH;
  int fallback = FALLBACK_NONE;
  double msBuild = 0;    // wall time of the BVH step alone
  double msKernels = 0;  // HIP-event time of the build kernels (kernel timing on), else 0
  double sahCost = 0;
};
// sum over all child boxes of area(child) / area(root) * (YRT_SAH_TRAV for an inner child, the
// triangle count for a leaf); 0 for an empty tree or a root without area
double bvh_sah_cost(const std::vector<GpuNode>& nodes);


}  // namespace yrt
