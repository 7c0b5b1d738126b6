// yrt_tri_record.h — the one writer of the per-triangle records GpuTri and GpuTriShade, called by
// the host builders (device/bvh_build.cpp, scene_gpu.cpp) and by the kernels (k_refit_tris, tri_at,
// postIntersect): the same bytes by construction (-ffp-contract=off on both sides), as yrt_qnode.h.
#pragma once

#include "yrt_gpu_types.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YRT_THD __host__ __device__ __forceinline__
#else
#define YRT_THD static inline
#endif

namespace yrt {

// e1 = p0 - p1, e2 = p2 - p0 (rtcore triangle convention): cross(e1, e2) is ray.Ng
YRT_THD void yrt_tri_edges(const float p0[3], const float p1[3], const float p2[3], float e1[3], float e2[3]) {
  for (int k = 0; k < 3; ++k) { e1[k] = p0[k] - p1[k]; e2[k] = p2[k] - p0[k]; }
}

// The leaf record's Moeller-Trumbore triangle; the .w words (id, flags, geometry) are left alone.
YRT_THD void yrt_tri_vertices(GpuTri& t, const float p0[3], const float p1[3], const float p2[3]) {
  for (int k = 0; k < 3; ++k) t.v0[k] = p0[k];
  yrt_tri_edges(p0, p1, p2, t.e1, t.e2);
}

// What moves with the vertices: the edges and the vertex normals (all the refit rewrites).
YRT_THD void yrt_tri_shade_vertices(GpuTriShade& r, const float p0[3], const float p1[3], const float p2[3],
                                    const float n0[3], const float n1[3], const float n2[3]) {
  yrt_tri_edges(p0, p1, p2, r.e1, r.e2);
  for (int k = 0; k < 3; ++k) { r.n[k] = n0[k]; r.n[3 + k] = n1[k]; r.n[6 + k] = n2[k]; }
}

// The whole record (zero normals / texcoords where the mesh has none).
YRT_THD void yrt_tri_shade_fill(GpuTriShade& r, const float p0[3], const float p1[3], const float p2[3],
                                const float n0[3], const float n1[3], const float n2[3], const float st0[2],
                                const float st1[2], const float st2[2], int32_t geom) {
  yrt_tri_shade_vertices(r, p0, p1, p2, n0, n1, n2);
  r.geom = geom;
  r.pad0 = r.pad1 = 0.f;
  for (int k = 0; k < 2; ++k) { r.st[k] = st0[k]; r.st[2 + k] = st1[k]; r.st[4 + k] = st2[k]; }
}

}  // namespace yrt
