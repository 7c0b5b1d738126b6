// k_refit.h — the BVH refit (faceCamera): triangle records, float node boxes, and their
// quantized copies.
#pragma once

#include "yrt_wave.h"
#include "../common/yrt_gpu_types.h"
#include "../common/yrt_qnode.h"
#include "../common/yrt_tri_record.h"

namespace yrt {

// ---------------------------------------------------------------- BVH refit (faceCamera)
// Per-face dynamic geometry (rtUpdatePrimitive of YULIO_CAMERA_ALIGNED_ meshes,
// singleray_device.cpp:354-398) keeps the BVH topology and only moves vertices: the moved
// triangles' Moeller-Trumbore records are rewritten from the new world vertices, then the
// node boxes are refit bottom-up, one launch per tree level (deepest first). The reference
// rebuilt the whole Embree BVH on every face commit. Boxes stay the exact
// union of the original vertex bounds (what the builder computes), so the hits are identical
// to a rebuild's: the closest hit is the smallest (t, triangle id) whatever the tree.
__global__ __launch_bounds__(YRT_BLOCK) void k_refit_tris(GpuTri* __restrict__ tris, GpuTriShade* __restrict__ triShade,
                                                         const int4* __restrict__ indices,
                                                         const float4* __restrict__ positions,
                                                         const float4* __restrict__ normals,
                                                         const int* __restrict__ leafStart,
                                                         const int* __restrict__ leafSlots, int firstTri, int numTris) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numTris) return;
  const int gid = firstTri + i;
  const int4 ix = indices[gid];
  const float4 a = positions[ix.x], b = positions[ix.y], c = positions[ix.z];
  const float4 na = normals[ix.x], nb = normals[ix.y], nc = normals[ix.z];
  // the host builder's functions: the shading record's edges and vertex normals (st, geom stay), and
  // every leaf slot referencing the triangle (spatial splits duplicate references; .w words kept)
  yrt_tri_shade_vertices(triShade[gid], &a.x, &b.x, &c.x, &na.x, &nb.x, &nc.x);
  for (int k = leafStart[gid]; k < leafStart[gid + 1]; ++k) yrt_tri_vertices(tris[leafSlots[k]], &a.x, &b.x, &c.x);
}

__global__ __launch_bounds__(YRT_BLOCK) void k_refit_nodes(GpuNode* __restrict__ nodes, const GpuTri* __restrict__ tris,
                                                          const int4* __restrict__ indices,
                                                          const float4* __restrict__ positions,
                                                          const int* __restrict__ levelNodes, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  GpuNode& n = nodes[levelNodes[i]];
  for (int k = 0; k < 4; ++k) {
    const int c = n.child[k];
    if (c == -1) continue;
    const int idx = c >> 5, cnt = c & 31;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (cnt > 0) {
      for (int t = 0; t < cnt; ++t) {
        const int gid = __float_as_int(tris[idx + t].v0[3]);
        const int4 ix = indices[gid];
        const float4 p[3] = {positions[ix.x], positions[ix.y], positions[ix.z]};
        for (int v = 0; v < 3; ++v) {
          lo[0] = fminf(lo[0], p[v].x); hi[0] = fmaxf(hi[0], p[v].x);
          lo[1] = fminf(lo[1], p[v].y); hi[1] = fmaxf(hi[1], p[v].y);
          lo[2] = fminf(lo[2], p[v].z); hi[2] = fmaxf(hi[2], p[v].z);
        }
      }
    } else {
      const GpuNode& ch = nodes[idx];
      for (int j = 0; j < 4; ++j) {
        if (ch.child[j] == -1) continue;
        lo[0] = fminf(lo[0], ch.lox[j]); hi[0] = fmaxf(hi[0], ch.hix[j]);
        lo[1] = fminf(lo[1], ch.loy[j]); hi[1] = fmaxf(hi[1], ch.hiy[j]);
        lo[2] = fminf(lo[2], ch.loz[j]); hi[2] = fmaxf(hi[2], ch.hiz[j]);
      }
    }
    n.lox[k] = lo[0]; n.hix[k] = hi[0];
    n.loy[k] = lo[1]; n.hiy[k] = hi[1];
    n.loz[k] = lo[2]; n.hiz[k] = hi[2];
  }
}

__global__ __launch_bounds__(YRT_BLOCK) void k_quantize_nodes(const GpuNode* __restrict__ nodes,
                                                             GpuQNode* __restrict__ qnodes, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  GpuQNode q;
  yrt_quantize_node(nodes[i], q);  // the host builder's function: the same bytes
  qnodes[i] = q;
}

}  // namespace yrt
