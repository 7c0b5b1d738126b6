// yrt_surface.h — what k_shade evaluates at a path vertex: postIntersect (the differential
// geometry of a hit), Material::shade (the BRDF components of the in-scope materials), the
// environment lights' radiance and Light::sample.
#pragma once

#include "yrt_shade.h"
#include "yrt_wave.h"
#include "../common/yrt_tri_record.h"

namespace yrt {

// ---------------------------------------------------------------- postIntersect
// BackendSceneFlat::postIntersect -> Shape::postIntersect, written once (post_intersect) over two
// vertex sources, which answer for a mesh triangle's edges, vertex normals, texture coordinates and
// interpolated tangents. The lazy and the indexed source load inside their accessors: only what
// the mesh's flags ask for. The burst source holds the whole record in registers.

// Record source: the triangle's 96-byte GpuTriShade, static meshes without tangent arrays. Its
// six 16-byte pieces r[0..5], all loaded by the caller (k_shade: in one group beside r[0], before
// the geometry record is known, so that a hit waits for its record once and not four times).
struct TriRecordSource {
  static constexpr bool kTangentArrays = false;
  float4 r[6];
  __device__ __forceinline__ void edges(V3& e1, V3& e2, V3& dPdu, V3& dPdv) const {
    e1 = v3(r[0].x, r[0].y, r[0].z); e2 = v3(r[1].x, r[1].y, r[1].z);
    dPdu = -e1; dPdv = e2;  // p1 - p0 but for a zero's sign: -0 where the indexed source has +0
  }
  __device__ __forceinline__ void normals(V3& n0, V3& n1, V3& n2) const {
    n0 = v3(r[2].x, r[2].y, r[2].z); n1 = v3(r[2].w, r[3].x, r[3].y); n2 = v3(r[3].z, r[3].w, r[4].x);
  }
  __device__ __forceinline__ void texcoords(float2& st0, float2& st1, float2& st2) const {
    st0 = make_float2(r[4].y, r[4].z); st1 = make_float2(r[4].w, r[5].x); st2 = make_float2(r[5].y, r[5].z);
  }
};

// The same record read piece by piece inside the accessors (rec), r0 = its first 16 bytes, which
// the caller has loaded for the geometry id: k_guides, off the render loop, and k_shade
// instantiations built without the record burst.
struct TriRecordLazySource {
  static constexpr bool kTangentArrays = false;
  const float4* __restrict__ rec;
  float4 r0;
  __device__ __forceinline__ void edges(V3& e1, V3& e2, V3& dPdu, V3& dPdv) const {
    const float4 r1 = rec[1];
    e1 = v3(r0.x, r0.y, r0.z); e2 = v3(r1.x, r1.y, r1.z);
    dPdu = -e1; dPdv = e2;
  }
  __device__ __forceinline__ void normals(V3& n0, V3& n1, V3& n2) const {
    const float4 r2 = rec[2], r3 = rec[3], r4 = rec[4];
    n0 = v3(r2.x, r2.y, r2.z); n1 = v3(r2.w, r3.x, r3.y); n2 = v3(r3.z, r3.w, r4.x);
  }
  __device__ __forceinline__ void texcoords(float2& st0, float2& st1, float2& st2) const {
    const float4 r4 = rec[4], r5 = rec[5];
    st0 = make_float2(r4.y, r4.z); st1 = make_float2(r4.w, r5.x); st2 = make_float2(r5.y, r5.z);
  }
};

// Indexed source: the index record and the vertex arrays, for moving meshes (GF_MOTION: vertices
// p + time * m, trianglemesh_full.cpp:211-215) and meshes with tangent arrays (tangent k: 0 Tx, 1 Ty).
struct TriIndexedSource {
  static constexpr bool kTangentArrays = true;
  const SceneView& sv;
  const int4 idx;
  const float time;
  const bool moving;
  __device__ __forceinline__ void edges(V3& e1, V3& e2, V3& dPdu, V3& dPdv) const {
    V3 p0 = ld3(sv.positions[idx.x]), p1 = ld3(sv.positions[idx.y]), p2 = ld3(sv.positions[idx.z]);
    if (moving) {
      p0 = p0 + time * ld3(sv.motions[idx.x]);
      p1 = p1 + time * ld3(sv.motions[idx.y]);
      p2 = p2 + time * ld3(sv.motions[idx.z]);
    }
    yrt_tri_edges(&p0.x, &p1.x, &p2.x, &e1.x, &e2.x);  // the record writers' (common/yrt_tri_record.h)
    dPdu = p1 - p0; dPdv = p2 - p0;
  }
  __device__ __forceinline__ void normals(V3& n0, V3& n1, V3& n2) const {
    n0 = ld3(sv.normals[idx.x]); n1 = ld3(sv.normals[idx.y]); n2 = ld3(sv.normals[idx.z]);
  }
  __device__ __forceinline__ void texcoords(float2& st0, float2& st1, float2& st2) const {
    st0 = sv.texcoords[idx.x]; st1 = sv.texcoords[idx.y]; st2 = sv.texcoords[idx.z];
  }
  __device__ __forceinline__ V3 tangent(int k, float w, float u, float v) const {
    return w * ld3(sv.tangents[2 * idx.x + k]) + u * ld3(sv.tangents[2 * idx.y + k]) +
           v * ld3(sv.tangents[2 * idx.z + k]);
  }
};

// The fields of a GpuGeom that post_intersect reads, held in registers (geom_burst below); Ng
// stays in memory, read by GEOM_TRIANGLE hits only.
struct GeomHead {
  int32_t kind, material, light, flags, illumMask, shadowMask;
  const float* Ng;
};

// geom: the hit triangle's geometry record (a GpuGeom or a GeomHead); rec: the record source of
// its GpuTriShade (TriRecordSource or TriRecordLazySource); (u, v): the hit's barycentrics; time:
// the ray's time.
template <class GEOM, class REC>
__device__ __forceinline__ void post_intersect(const SceneView& sv, const GEOM& geom, const REC& rec, V3 org, V3 dir,
                                               float t, float u, float v, int gid, DG& dg, bool wantTangents,
                                               float time) {
  dg.material = geom.material;
  dg.light = geom.light;
  dg.illumMask = geom.illumMask;
  dg.shadowMask = geom.shadowMask;
  dg.P = org + t * dir;
  dg.s = u; dg.t = v;  // unless the mesh has texture coordinates
  dg.Tx = dg.Ty = v3s(0.f);
  auto mesh = [&](const auto src) {  // TriangleMeshFull / TriangleMeshWithNormals::postIntersect
    V3 e1, e2, dPdu, dPdv;
    src.edges(e1, e2, dPdu, dPdv);
    const float w = 1.0f - u - v;
    dg.Ns = dg.Ng = normalize(cross(e1, e2));  // ray.Ng (unnormalized Embree Ng)
    const bool meshNormals = geom.kind == GEOM_MESH_NORMALS;
    if (meshNormals || (geom.flags & GF_NORMALS)) {
      V3 n0, n1, n2;
      src.normals(n0, n1, n2);
      V3 Ns = w * n0 + u * n1 + v * n2;
      const float len2 = dot(Ns, Ns);
      Ns = len2 > 0 ? Ns * rsqrtf_(len2) : dg.Ng;
      if (dot(Ns, dg.Ng) < 0) Ns = -Ns;
      dg.Ns = Ns;
    }
    if (meshNormals) {  // shapes/trianglemesh_normals.cpp:125-147
      dg.Tx = dPdu; dg.Ty = dPdv;
      return;
    }
    // shapes/trianglemesh_full.cpp:192-260
    float dsdu = 1, dtdu = 0, dsdv = 0, dtdv = 1;
    if (geom.flags & GF_TEXCOORDS) {
      float2 st0, st1, st2;
      src.texcoords(st0, st1, st2);
      dg.s = st0.x * w + st1.x * u + st2.x * v;
      dg.t = st0.y * w + st1.y * u + st2.y * v;
      dsdu = st1.x - st0.x; dtdu = st1.y - st0.y;
      dsdv = st2.x - st0.x; dtdv = st2.y - st0.y;
    }
    if (!wantTangents) return;
    // trianglemesh_full.cpp:244-263: derived tangents, interpolated ones where the mesh has them
    const V3 dPds = normalize(dPdu * dtdv - dPdv * dtdu);
    dg.Tx = normalize(dPds - dot(dPds, dg.Ns) * dg.Ns);
    const V3 dPdt = normalize(dPdv * dsdu - dPdu * dsdv);
    dg.Ty = normalize(dPdt - dot(dPdt, dg.Ns) * dg.Ns);
    if constexpr (src.kTangentArrays) {
      if (geom.flags & GF_TANGENT_X) dg.Tx = src.tangent(0, w, u, v);
      if (geom.flags & GF_TANGENT_Y) dg.Ty = src.tangent(1, w, u, v);
    }
  };
  // the one place that picks the source: the vertex arrays for moving meshes and tangent arrays
  if (geom.kind == GEOM_TRIANGLE)  // shapes/triangle.h:69-78
    dg.Ns = dg.Ng = v3(geom.Ng[0], geom.Ng[1], geom.Ng[2]);
  else if (geom.flags & (GF_MOTION | GF_TANGENT_X | GF_TANGENT_Y))
    mesh(TriIndexedSource{sv, sv.indices[gid], time, (geom.flags & GF_MOTION) != 0});
  else
    mesh(rec);
  dg.error = fmaxf(fabsf(t), reduce_max(absv(dg.P)));
}

// ---------------------------------------------------------------- the geometry record in one group
// What an instantiation's shade_material cases and post_intersect read of a hit's GpuGeomRec,
// issued as 16-byte loads in one group when the geometry id is known: the record is 13 such
// pieces (q), all inside the one record, and shade_material then selects among registers in
// place of loading a field, waiting, branching on it and loading the next.
//   q0 q1   GpuGeom: kind, material, light, flags | vtxBase, triBase, illumMask, shadowMask
//   q2      GpuGeom::Ng (GEOM_TRIANGLE only: left in memory)
//   q3      m.type, m.tex[0..2]        q4  m.tex[3..4], m.media[0..1]
//   q5..q10 m.p[0..23]                 q11 q12  t0
// number of leading p[] pieces the material types of MM read (the cases of shade_material)
template <unsigned MM>
constexpr int mat_p_quads() {
  int n = 0;
  constexpr unsigned one = mat_bit(MAT_MATTE) | mat_bit(MAT_MIRROR) | mat_bit(MAT_MATTE_TEXTURED);            // p[0..3]
  constexpr unsigned two = mat_bit(MAT_VELVET) | mat_bit(MAT_OBJ) | mat_bit(MAT_METALLIC_PAINT);             // p[0..7]
  constexpr unsigned three = mat_bit(MAT_PLASTIC) | mat_bit(MAT_DIELECTRIC) | mat_bit(MAT_METAL) |
                             mat_bit(MAT_METALLIC_GLITTER) | mat_bit(MAT_UBER) | mat_bit(MAT_THIN_DIELECTRIC);  // p[0..11]
  constexpr unsigned four = mat_bit(MAT_BRUSHED_METAL);                                                       // p[0..12]
  if (MM & one) n = 1;
  if (MM & two) n = 2;
  if (MM & three) n = 3;
  if (MM & four) n = 4;
  return n;
}
// the material types that read tex[3..4] or media[] (q4), and those that sample tex[0] through t0
constexpr unsigned kMatsQ4 = mat_bit(MAT_OBJ) | mat_bit(MAT_DIELECTRIC);
constexpr unsigned kMatsT0 = mat_bit(MAT_MATTE_TEXTURED) | mat_bit(MAT_OBJ) | mat_bit(MAT_UBER) | mat_bit(MAT_THIN_DIELECTRIC);

// m and t0 are written only where MM's materials read them; the rest keeps the caller's zeros.
template <unsigned MM>
__device__ __forceinline__ void geom_burst(const GpuGeomRec* __restrict__ gr, GeomHead& gh, GpuMaterial& m,
                                           GpuTexture& t0) {
  static_assert(sizeof(GpuGeom) == 48 && sizeof(GpuMaterial) == 128 && sizeof(GpuGeomRec) == 208, "piece offsets below");
  const int4* __restrict__ q = (const int4*)gr;
  constexpr int NP = mat_p_quads<MM>();
  const int4 q0 = q[0], q1 = q[1], q3 = q[3];
  int4 q4 = make_int4(0, 0, 0, 0), qt0 = q4, qt1 = q4;
  float4 qp[4];
  if constexpr ((MM & kMatsQ4) != 0u) q4 = q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) qp[k] = k < NP ? ((const float4*)gr)[5 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr ((MM & kMatsT0) != 0u) { qt0 = q[11]; qt1 = q[12]; }
  gh.kind = q0.x; gh.material = q0.y; gh.light = q0.z; gh.flags = q0.w;
  gh.illumMask = q1.z; gh.shadowMask = q1.w;
  gh.Ng = gr->g.Ng;
  m.type = q3.x; m.tex[0] = q3.y; m.tex[1] = q3.z; m.tex[2] = q3.w;
  if constexpr ((MM & kMatsQ4) != 0u) { m.tex[3] = q4.x; m.tex[4] = q4.y; m.media[0] = q4.z; m.media[1] = q4.w; }
#pragma unroll
  for (int k = 0; k < NP; ++k) { m.p[4 * k] = qp[k].x; m.p[4 * k + 1] = qp[k].y; m.p[4 * k + 2] = qp[k].z; m.p[4 * k + 3] = qp[k].w; }
  if constexpr ((MM & kMatsT0) != 0u) {
    t0.image = qt0.x; t0.filter = qt0.y; t0.invert = qt0.z; t0.width = qt0.w;
    t0.height = qt1.x; t0.format = qt1.y;
    t0.offset = (int64_t)(((uint64_t)(uint32_t)qt1.w << 32) | (uint32_t)qt1.z);
  }
}

__device__ __forceinline__ void add_comp(BRDFSet& bs, int kind, uint32_t type, V3 R, float a = 0.f, float b = 0.f,
                                         float c = 0.f) {
  (void)type;  // == comp_type(kind), documented at each call
  // Unconditional constant-index stores of selected values: a conditional store lets the
  // optimizer merge the slots into a pointer phi, which pins the set in scratch memory.
#pragma unroll
  for (int i = 0; i < YRT_MAX_COMPS; ++i) {
    const bool w = i == bs.n;
    bs.c[i].kind = w ? kind : bs.c[i].kind;
    bs.c[i].R = v3(w ? R.x : bs.c[i].R.x, w ? R.y : bs.c[i].R.y, w ? R.z : bs.c[i].R.z);
    bs.c[i].a = w ? a : bs.c[i].a;
    bs.c[i].b = w ? b : bs.c[i].b;
    bs.c[i].c = w ? c : bs.c[i].c;
  }
  bs.n = bs.n < YRT_MAX_COMPS ? bs.n + 1 : bs.n;
}

// Material::shade for the in-scope materials (materials/*.h). May modify dg.Ns (Obj bump).
template <unsigned MM>
// t0: the descriptor of m.tex[0] (GpuGeomRec::t0)
__device__ __forceinline__ void shade_material(const SceneView& sv, const GpuMaterial& m, const GpuTexture& t0, int matId,
                                               int medium, DG& dg, BRDFSet& bs) {
  bs.n = 0;
  // each case is compiled only when the instantiation's material set MM holds its type
  const float idBits = __int_as_float(matId);
  switch (m.type) {
    case MAT_PLASTIC:
      if constexpr (!(MM & mat_bit(MAT_PLASTIC))) break;
      // p: pigment[0..2], eta[3], roughness[4], rcpRoughness[5], layer etait[6], etati[7], eta_[8]
      add_comp(bs, C_DIEL_LAYER_LAMB, BT_DIFFUSE_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[6], m.p[7]);
      if (m.p[4] == 0.0f) add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[8], 1.0f);
      else add_comp(bs, C_MICROFACET, BT_GLOSSY_REFLECTION, v3s(1.f), 1.0f, m.p[3], m.p[5]);
      break;
    case MAT_DIELECTRIC:
      if constexpr (!(MM & mat_bit(MAT_DIELECTRIC))) break;
      // outside -> inside when the ray travels in the outside medium (dielectric.h:42-52)
      if (medium == m.media[0]) {
        add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[8], 1.0f);
        add_comp(bs, C_DIEL_TRANS, BT_SPECULAR_TRANSMISSION, v3s(0.f), m.p[8]);
      } else {
        add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[9], 1.0f);
        add_comp(bs, C_DIEL_TRANS, BT_SPECULAR_TRANSMISSION, v3s(0.f), m.p[9]);
      }
      break;
    case MAT_MIRROR:
      if constexpr (!(MM & mat_bit(MAT_MIRROR))) break;
      add_comp(bs, C_REFLECTION, BT_SPECULAR_REFLECTION, v3(m.p[0], m.p[1], m.p[2]));
      break;
    case MAT_METAL:
      if constexpr (!(MM & mat_bit(MAT_METAL))) break;
      // p: R[0..2], eta[3..5], k[6..8], roughness[9], rcpRoughness[10]
      if (m.p[9] == 0.0f) add_comp(bs, C_CONDUCTOR, BT_SPECULAR_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), 0.f, 0.f, idBits);
      else add_comp(bs, C_MICRO_COND, BT_GLOSSY_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[10], 0.f, idBits);
      break;
    case MAT_BRUSHED_METAL:
      if constexpr (!(MM & mat_bit(MAT_BRUSHED_METAL))) break;
      // p: R[0..2], eta[3..5], k[6..8], roughnessX[9], roughnessY[10], rcp[11], rcp[12]
      if (m.p[9] == 0.0f || m.p[10] == 0.0f)
        add_comp(bs, C_CONDUCTOR, BT_SPECULAR_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), 0.f, 0.f, idBits);
      else
        add_comp(bs, C_MICRO_ANISO, BT_GLOSSY_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[11], m.p[12], idBits);
      break;
    case MAT_VELVET:
      if constexpr (!(MM & mat_bit(MAT_VELVET))) break;
      add_comp(bs, C_MINNAERT, BT_DIFFUSE_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[3]);
      add_comp(bs, C_VELVETY, BT_DIFFUSE_REFLECTION, v3(m.p[4], m.p[5], m.p[6]), m.p[7]);
      break;
    case MAT_MATTE:
      if constexpr (!(MM & mat_bit(MAT_MATTE))) break;
      add_comp(bs, C_LAMBERT, BT_DIFFUSE_REFLECTION, v3(m.p[0], m.p[1], m.p[2]));
      break;
    case MAT_MATTE_TEXTURED:
      if constexpr (!(MM & mat_bit(MAT_MATTE_TEXTURED))) break;
      if (m.tex[0] >= 0) {
        float c[4];
        tex_get_rec(t0, sv.texels, sv.texQuads, m.p[2] * dg.s + m.p[0], m.p[3] * dg.t + m.p[1], c);
        add_comp(bs, C_LAMBERT, BT_DIFFUSE_REFLECTION, v3(c[0], c[1], c[2]));
      }
      break;
    case MAT_METALLIC_PAINT:
      if constexpr (!(MM & mat_bit(MAT_METALLIC_PAINT))) break;
      // p: shadeColor[0..2], eta[3], reflection eta_ [4], layer etait [5], etati [6]
      add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[4], 1.0f);
      add_comp(bs, C_DIEL_LAYER_LAMB, BT_DIFFUSE_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[5], m.p[6]);
      break;
    case MAT_METALLIC_GLITTER:
      if constexpr (!(MM & mat_bit(MAT_METALLIC_GLITTER))) break;
      // MetallicPaint::shade (metallicpaint.h:58-71); p as above + glitterColor [7..9], n = 1/spread [10]
      add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[4], 1.0f);
      add_comp(bs, C_DIEL_LAYER_LAMB, BT_DIFFUSE_REFLECTION, v3(m.p[0], m.p[1], m.p[2]), m.p[5], m.p[6]);
      add_comp(bs, C_DIEL_LAYER_GLITTER, BT_GLOSSY_REFLECTION, v3(m.p[7], m.p[8], m.p[9]), m.p[5], m.p[6], m.p[10]);
      break;
    case MAT_OBJ: {
      if constexpr (!(MM & mat_bit(MAT_OBJ))) break;
      // p: d[0], Kd[1..3], Ks[4..6], Ns[7]; tex: map_d, map_Kd, map_Ks, map_Ns, map_Bump
      float c[4];
      if (m.tex[4] >= 0) {
        tex_get(sv.textures, sv.images, sv.texels, sv.texQuads, m.tex[4], dg.s, dg.t, c);
        const V3 b = v3(2.0f * c[0] - 1.0f, 2.0f * c[1] - 1.0f, 2.0f * c[2] - 1.0f);
        dg.Ns = normalize(b.x * dg.Tx + b.y * dg.Ty + b.z * dg.Ns);
      }
      float d = m.p[0];
      if (m.tex[0] >= 0) {
        tex_get_rec(t0, sv.texels, sv.texQuads, dg.s, dg.t, c);
        d *= c[0];
      }
      if (d < 1.0f) add_comp(bs, C_TRANSMISSION, BT_SPECULAR_TRANSMISSION, v3s(1.0f - d));
      V3 Kd = d * v3(m.p[1], m.p[2], m.p[3]);
      if (m.tex[1] >= 0) {
        tex_get(sv.textures, sv.images, sv.texels, sv.texQuads, m.tex[1], dg.s, dg.t, c);
        Kd = Kd * v3(c[0], c[1], c[2]);
      }
      if (Kd != v3s(0.f)) add_comp(bs, C_LAMBERT, BT_DIFFUSE_REFLECTION, Kd);
      float Ns = m.p[7];
      if (m.tex[3] >= 0) {
        tex_get(sv.textures, sv.images, sv.texels, sv.texQuads, m.tex[3], dg.s, dg.t, c);
        Ns *= c[0];
      }
      V3 Ks = d * v3(m.p[4], m.p[5], m.p[6]);
      if (m.tex[2] >= 0) {
        tex_get(sv.textures, sv.images, sv.texels, sv.texQuads, m.tex[2], dg.s, dg.t, c);
        Ks = Ks * v3(c[0], c[1], c[2]);
      }
      if (Ks != v3s(0.f)) add_comp(bs, C_SPECULAR, BT_GLOSSY_REFLECTION, Ks, Ns);
      break;
    }
    case MAT_UBER: {
      if constexpr (!(MM & mat_bit(MAT_UBER))) break;
      // p: diffuse[0..2], s0[3..4], ds[5..6], eta[7], roughness[8], reflectivity[9],
      //    rcpRoughness[10], eta_ = 1*rcp(eta) [11]
      float dc[4] = {m.p[0], m.p[1], m.p[2], 1.f};
      float alpha = 1.f, opacity = 0.f;
      if (m.tex[0] >= 0) {
        tex_get_rec(t0, sv.texels, sv.texQuads, m.p[5] * dg.s + m.p[3], m.p[6] * dg.t + m.p[4], dc);
        alpha = dc[3];
        opacity = 1.f - alpha;
      }
      add_comp(bs, C_LAMBERT, BT_DIFFUSE_REFLECTION, v3(dc[0] * alpha, dc[1] * alpha, dc[2] * alpha));
      if (alpha < 1.f) add_comp(bs, C_CONST_DIEL_TRANS, BT_SPECULAR_TRANSMISSION, v3s(opacity));
      if (m.p[9] > 0.f) add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[11], alpha * m.p[9]);
      else if (m.p[8] == 0.f) add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[11], alpha);
      else add_comp(bs, C_MICROFACET, BT_GLOSSY_REFLECTION, v3s(alpha), 1.f, m.p[7], m.p[10]);
      break;
    }
    case MAT_THIN_DIELECTRIC: {
      if constexpr (!(MM & mat_bit(MAT_THIN_DIELECTRIC))) break;
      // p: transmission[0..2], s0[3..4], ds[5..6], eta[7], thickness[8], transparency[9], eta_[10]
      add_comp(bs, C_DIEL_REFL, BT_SPECULAR_REFLECTION, v3s(0.f), m.p[10], 1.0f);
      float dc[4] = {m.p[0], m.p[1], m.p[2], 1.f};
      if (m.tex[0] >= 0)
        tex_get_rec(t0, sv.texels, sv.texQuads, m.p[5] * dg.s + m.p[3], m.p[6] * dg.t + m.p[4], dc);
      const float tr = m.p[9];
      const V3 T = v3(dc[0] * tr, dc[1] * tr, dc[2] * tr);
      add_comp(bs, C_THIN_DIEL_TRANS, BT_SPECULAR_TRANSMISSION, v3(yrt_logf(T.x), yrt_logf(T.y), yrt_logf(T.z)), m.p[10],
               m.p[8]);
      break;
    }
    default:
      break;
  }
}

__device__ __forceinline__ void img_get(const SceneView& sv, int image, int x, int y, float c[4]) {
  texel(sv.images[image], sv.texels, x, y, c);
}

// HDRILight::Le (lights/hdrilight.cpp:43-71)
template <class LT>  // GpuLight, or a YRT_CONST one (scalar loads)
__device__ __forceinline__ V3 hdri_Le(const SceneView& sv, const LT& lt, V3 wo) {
  const A3 w2l = ldA3(lt.w2l);
  const V3 wi = xfmVector(w2l, -wo);
  const float theta = yrt_acosf(clampf(wi.y, -1.0f, 1.0f));
  float phi = yrt_atan2f(-wi.z, -wi.x);
  if (phi < 0) phi += 2.0f * kPi;
  const float u = 1.0f - (phi * kOneOverTwoPi);
  const float v = theta * kOneOverPi;
  const int width = lt.hdriW, height = lt.hdriH;
  int x = max(0, min((int)(u * width), width - 1));
  int xNext = x + 1;
  if (xNext == width) xNext = 0;
  const float alpha = u * width - x;
  int y = max(0, min((int)(v * height), height - 1));
  int yNext = y + 1;
  if (yNext == height) yNext = height - 1;
  const float beta = v * height - y;
  float c0[4], c1[4], c2[4], c3[4];
  img_get(sv, lt.image, x, y, c0);
  img_get(sv, lt.image, xNext, y, c1);
  img_get(sv, lt.image, xNext, yNext, c2);
  img_get(sv, lt.image, x, yNext, c3);
  V3 r;
  float* rr = &r.x;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float temp0 = beta * c3[k] + (1 - beta) * c0[k];
    const float temp1 = beta * c2[k] + (1 - beta) * c1[k];
    rr[k] = lt.L[k] * (alpha * temp1 + (1 - alpha) * temp0);
  }
  return r;
}

// LM: the light types (bit LIGHT_x) an instantiation handles: bits 16.. of the shade kernel's
// instantiation mask (light_bit), which the launcher picks as a superset of the scene's lights.
constexpr unsigned kAllLights = 0x7Fu;
template <unsigned MM>
constexpr unsigned lights_of() { return (MM >> 16) & kAllLights; }
template <unsigned LM, class LT>
__device__ __forceinline__ V3 env_Le(const SceneView& sv, const LT& lt, V3 wo) {
  if ((LM & (1u << LIGHT_AMBIENT)) && lt.type == LIGHT_AMBIENT) return v3(lt.L[0], lt.L[1], lt.L[2]);
  if ((LM & (1u << LIGHT_DISTANT)) && lt.type == LIGHT_DISTANT)  // DistantLight::Le (distantlight.h:38-41)
    return dot(-wo, ld3(lt.e1)) >= lt.bsphere[1] ? v3(lt.L[0], lt.L[1], lt.L[2]) : v3s(0.f);
  if ((LM & (1u << LIGHT_HDRI)) && lt.type == LIGHT_HDRI) return hdri_Le(sv, lt, wo);
  return v3s(0.f);
}

// the light types whose sample() reads the raw 2-D sample (sx, sy), and those that read its
// tabulated terms sd (the point, spot and directional lights read neither)
constexpr unsigned kLightsRawS = (1u << LIGHT_TRIANGLE) | (1u << LIGHT_DISTANT);
constexpr unsigned kLightsDir = (1u << LIGHT_AMBIENT) | (1u << LIGHT_DISTANT);
// Light::sample for a non-precomputed light at the 2-D sample (sx, sy), sd = sample_dir(sx, sy);
// returns L, sets wi/pdf.
template <unsigned LM, class LT>
__device__ __forceinline__ V3 light_sample(const LT& lt, const DG& dg, float4 sd, float sx, float sy, V3& wi,
                                           float& pdf) {
  if ((LM & (1u << LIGHT_AMBIENT)) && lt.type == LIGHT_AMBIENT) {
    // lights/ambientlight.h:52-65 (the bsphere tMax is overwritten by the integrator)
    wi = cosine_hemi_dg(sd, dg, pdf);
    return v3(lt.L[0], lt.L[1], lt.L[2]);
  }
  if ((LM & (1u << LIGHT_TRIANGLE)) && lt.type == LIGHT_TRIANGLE) {
    // lights/trianglelight.h:77-85
    const V3 A = ld3(lt.v0), B = ld3(lt.v1), C = ld3(lt.v2);
    const float su = sqrtf(sx);
    const V3 d = (C + (1.0f - su) * (A - C) + (sy * su) * (B - C)) - dg.P;
    const float tMax = length(d);
    const float dDotNg = dot(d, ld3(lt.Ng));
    if (dDotNg >= 0) {
      pdf = 0.f;
      wi = v3s(0.f);
      return v3s(0.f);
    }
    wi = d * rcpf_(tMax);
    pdf = 2.0f * tMax * tMax * tMax * rcpf_(fabsf(dDotNg));
    return v3(lt.L[0], lt.L[1], lt.L[2]);
  }
  if ((LM & (1u << LIGHT_POINT)) && lt.type == LIGHT_POINT) {  // pointlight.h:36-42
    const V3 d = ld3(lt.v0) - dg.P;
    const float distance = length(d);
    wi = d / distance;
    pdf = distance * distance;
    return v3(lt.L[0], lt.L[1], lt.L[2]);
  }
  if ((LM & (1u << LIGHT_SPOT)) && lt.type == LIGHT_SPOT) {  // spotlight.h:41-52
    const V3 d = ld3(lt.v0) - dg.P;
    const float distance = length(d);
    wi = d * rcpf_(distance);
    pdf = distance * distance;
    const float cosAngle = dot(wi, ld3(lt.e1));
    const float cosMin = lt.bsphere[0], cosMax = lt.bsphere[1];
    if (cosMin != cosMax) return v3(lt.L[0], lt.L[1], lt.L[2]) * clampf((cosAngle - cosMax) * rcpf_(cosMin - cosMax));
    if (cosAngle > cosMin) return v3(lt.L[0], lt.L[1], lt.L[2]);
    return v3s(0.f);
  }
  if ((LM & (1u << LIGHT_DIRECTIONAL)) && lt.type == LIGHT_DIRECTIONAL) {  // directionallight.h:31-33 (Sample3f pdf defaults to 1)
    wi = ld3(lt.e1);
    pdf = 1.0f;
    return v3(lt.L[0], lt.L[1], lt.L[2]);
  }
  if ((LM & (1u << LIGHT_DISTANT)) && lt.type == LIGHT_DISTANT) {  // distantlight.h:46-50, uniformSampleCone (shapesampler.h:149-165)
    const float angle = lt.bsphere[0];
    const float cosTheta = 1.0f - sy * (1.0f - yrt_cosf(angle));
    const float sinTheta = cos2sin(cosTheta);
    const V3 l = v3(sd.x * sinTheta, sd.y * sinTheta, cosTheta);
    pdf = rcpf_(4.0f * kPi * sqrf(yrt_sinf(0.5f * angle)));
    wi = mul(frame(ld3(lt.e1)), l);
    return v3(lt.L[0], lt.L[1], lt.L[2]);
  }
  pdf = 0.f;
  wi = v3s(0.f);
  return v3s(0.f);
}

}  // namespace yrt
