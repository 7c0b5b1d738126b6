// scene_gpu.cpp — flatten a committed scene into HBM buffers + BVH.
//
// Follows BackendSceneFlat::Handle::create (api/scene_flat.h:72-97) and the
// BackendSceneFlat ctor (:105-121): geomID = index among primitives that have a shape, in
// slot order; allLights in slot order; envLights = ambient/HDRI lights. Geometry is the
// world-space result of Shape::transform, exactly what extract() handed to Embree.
//
// build_gpu_scene runs the stages below in turn; a host-only scene skips the two that need a
// device. The device buffers are listed once, in SceneBuffers (scene_gpu.h).
#include "scene_gpu.h"

#include <string.h>

#include <chrono>
#include <map>

#include "../common/yrt_tri_record.h"
#include "distribution.h"

namespace yrt {

using Prims = std::vector<std::shared_ptr<ScenePrim>>;

template <class V>  // V3 or float4
static void st3(float* d, const V& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }

// SceneView pointers of the scene's own device buffers: the one place that gives them their types
static void bind_view(GpuScene& S) {
  SceneView& v = S.view;
  v.qnodes = S.qnodes.as<GpuQNode>();
  v.tris = S.tris.as<GpuTri>();
  v.triGeom = S.triGeom.as<int>();
  v.indices = S.indices.as<int4>();
  v.positions = S.positions.as<float4>();
  v.normals = S.normals.as<float4>();
  v.texcoords = S.texcoords.as<float2>();
  v.geoms = S.geoms.as<GpuGeom>();
  v.geomRecs = S.geomRecs.as<GpuGeomRec>();
  v.triShade = S.triShade.as<GpuTriShade>();
  v.materials = S.materials.as<GpuMaterial>();
  v.textures = S.textures.as<GpuTexture>();
  v.images = S.images.as<GpuImage>();
  v.texels = S.texels.as<uint8_t>();
  v.texQuads = S.texQuads.as<uint8_t>();
  v.lights = S.lights.as<GpuLight>();
  v.envLights = S.envLights.as<int>();
  v.media = S.media.as<float4>();
  v.motions = S.motions.as<float4>();
  v.tangents = S.tangents.as<float4>();
  v.triMotion = S.triMotion.as<GpuTriMotion>();
  v.hdriDist = nullptr;  // no buffer behind it: the field only keeps the kernel argument's layout
}

// The device record of a world-space light, without the scene's own indices (image, precomputed
// slot, environment list): what the light samplers read.
GpuLight gpu_light_record(const LightInst& L) {
  GpuLight g;
  memset(&g, 0, sizeof(g));
  g.type = L.type;
  g.illumMask = L.illumMask;
  g.shadowMask = L.shadowMask;
  g.precomputed = -1;
  g.L[0] = L.L.x; g.L[1] = L.L.y; g.L[2] = L.L.z;
  st3(g.v0, L.v0); st3(g.v1, L.v1); st3(g.v2, L.v2);
  st3(g.e1, L.e1); st3(g.e2, L.e2); st3(g.Ng, L.Ng);
  auto stA = [](float* d, const A3& a) {
    const float v[12] = {a.l.vx.x, a.l.vx.y, a.l.vx.z, a.l.vy.x, a.l.vy.y, a.l.vy.z,
                         a.l.vz.x, a.l.vz.y, a.l.vz.z, a.p.x,    a.p.y,    a.p.z};
    memcpy(d, v, sizeof(v));
  };
  stA(g.l2w, L.l2w);
  stA(g.w2l, L.w2l);
  g.bsphere[0] = L.type == LIGHT_SPOT ? L.cosAngleMin : L.halfAngle;
  g.bsphere[1] = L.type == LIGHT_SPOT ? L.cosAngleMax : L.cosHalfAngle;
  return g;
}

// Bilinear footprints of the 8-bit images (kernels/yrt_shade.h tex_get_rec): record i of an image,
// i = y W + x, holds the 4-byte texels (x, y), (x', y), (x, y'), (x', y') with x' = min(x + 1, W - 1)
// and y' = min(y + 1, H - 1), at 4x the texel's byte offset: the bytes the four row-major fetches
// read, of its own image only. Float images keep the row-major pool only.
std::vector<uint32_t> build_tex_quads(const std::vector<GpuImage>& images, const std::vector<uint8_t>& texels,
                                      size_t texels8Bytes) {
  std::vector<uint32_t> quads(texels8Bytes, 0u);
  for (const GpuImage& g : images) {
    if (g.format == IMG_RGBAF32) continue;
    const size_t W = (size_t)g.width, H = (size_t)g.height;
    auto word = [&](size_t x, size_t y) -> uint32_t {
      uint32_t w;
      memcpy(&w, &texels[(size_t)g.offset + 4 * (y * W + x)], 4);
      return w;
    };
    for (size_t y = 0; y < H; ++y)
      for (size_t x = 0; x < W; ++x) {
        const size_t q = (size_t)g.offset + 4 * (y * W + x);  // uint32 index of the record = byte offset
        const size_t x1 = std::min(x + 1, W - 1), y1 = std::min(y + 1, H - 1);
        quads[q + 0] = word(x, y);
        quads[q + 1] = word(x1, y);
        quads[q + 2] = word(x, y1);
        quads[q + 3] = word(x1, y1);
      }
  }
  return quads;
}

static float4 f4(V3 v) { return make_float4(v.x, v.y, v.z, 0.f); }
// n vertices of a mesh attribute as the device's float4s; zeros for an attribute the mesh lacks
static void append_f4(std::vector<float4>& dst, const std::vector<V3>& src, size_t n) {
  const size_t o = dst.size();
  dst.resize(o + n, make_float4(0.f, 0.f, 0.f, 0.f));
  if (!src.empty())
    for (size_t k = 0; k < n; ++k) dst[o + k] = f4(src[k]);
}

// The scene bounds: over the vertices the triangles reference, in slot and triangle order
static void scene_bounds(const Prims& prims, float lo[3], float hi[3]) {
  for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
  for (const auto& p : prims) {
    if (!p || !p->shape) continue;
    const MeshInst& m = *p->shape;
    for (int v : m.tri) {
      const float c[3] = {m.pos[v].x, m.pos[v].y, m.pos[v].z};
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], c[k]); hi[k] = std::max(hi[k], c[k]); }
    }
  }
}

// Stage 1, flatten: the host tables of a scene as they are uploaded, filled from the slots without a HIP call.
// Materials, textures and images are deduplicated by object, media by value.
struct SceneTables {
  std::vector<float4> positions, normals, motions, tangents;  // tangents: (x, y) per vertex
  std::vector<float2> texcoords;
  std::vector<int4> indices;
  std::vector<float> triVerts, triVerts1;  // triVerts1 (moving scenes): the triangles at the end of the frame time
  std::vector<uint32_t> triFlags;
  std::vector<int> triGeom, envLights, primLight;  // primLight: slot -> its light, or -1
  std::vector<GpuGeom> geoms;
  std::vector<GpuMaterial> materials;
  std::vector<GpuTexture> textures;
  std::vector<GpuImage> images;
  // 8-bit images first, float images (HDRI maps) after them: the bilinear footprint records
  // (texQuads, 4x the bytes) cover only the 8-bit part of the pool, texels8Bytes
  std::vector<uint8_t> texels, texelsF;
  size_t texels8Bytes = 0;
  // medium table (materials/medium.h): [0] = vacuum; Medium::operator== compares by value, so
  // media are deduplicated by value and compared by index on the GPU
  std::vector<float4> media = {make_float4(1.f, 1.f, 1.f, 1.f)};
  std::vector<GpuLight> lights;
  std::vector<std::shared_ptr<const LightInst>> allLights;
  std::vector<LightSampleSource> precomputed;
  std::map<const MaterialInst*, int> matIds;
  std::map<const TextureInst*, int> texIds;
  std::map<const ImageObj*, int> imgIds;
  int numEnvZero = 0, numEnvDir = 0, numTris = 0;
  bool anyMotion = false, anyTangent = false;

  explicit SceneTables(const Prims& prims) { add_lights(prims); add_geoms(prims); place_float_texels(); }
  void add_lights(const Prims& prims);
  void add_geoms(const Prims& prims);
  void place_float_texels();

  int imageId(const std::shared_ptr<ImageObj>& im) {
    auto it = imgIds.find(im.get());
    if (it != imgIds.end()) return it->second;
    GpuImage g;
    memset(&g, 0, sizeof(g));
    g.width = im->width; g.height = im->height; g.format = im->format;
    std::vector<uint8_t>& pool = im->format == IMG_RGBAF32 ? texelsF : texels;
    size_t off = (pool.size() + 15) & ~size_t(15);
    pool.resize(off);
    g.offset = (int64_t)off;  // float images: relative to the float part until it is placed
    pool.insert(pool.end(), im->data.begin(), im->data.end());
    images.push_back(g);
    return imgIds[im.get()] = (int)images.size() - 1;
  }
  int textureId(const std::shared_ptr<const TextureInst>& t) {
    if (!t) return -1;
    auto it = texIds.find(t.get());
    if (it != texIds.end()) return it->second;
    GpuTexture g;
    memset(&g, 0, sizeof(g));
    g.image = imageId(t->image);
    const GpuImage& im = images[g.image];
    g.width = im.width; g.height = im.height; g.format = im.format; g.offset = im.offset;
    g.filter = t->filter;
    g.invert = t->invert ? 1 : 0;
    textures.push_back(g);
    return texIds[t.get()] = (int)textures.size() - 1;
  }
  int mediumId(float tr, float tg, float tb, float eta) {
    for (size_t i = 0; i < media.size(); ++i)
      if (media[i].x == tr && media[i].y == tg && media[i].z == tb && media[i].w == eta) return (int)i;
    media.push_back(make_float4(tr, tg, tb, eta));
    return (int)media.size() - 1;
  }
  int materialId(const std::shared_ptr<const MaterialInst>& m) {
    if (!m) return -1;
    auto it = matIds.find(m.get());
    if (it != matIds.end()) return it->second;
    GpuMaterial g = m->gm;
    for (int k = 0; k < 5; ++k) g.tex[k] = textureId(m->tex[k]);
    if (g.type == MAT_DIELECTRIC) {
      g.media[0] = mediumId(g.p[0], g.p[1], g.p[2], g.p[3]);  // outside
      g.media[1] = mediumId(g.p[4], g.p[5], g.p[6], g.p[7]);  // inside
    }
    materials.push_back(g);
    return matIds[m.get()] = (int)materials.size() - 1;
  }
};

// HDRILight::sample (lights/hdrilight.cpp:77-87), evaluated once per sample record
static LightSampleSource hdri_sample_source(std::shared_ptr<const LightInst> lp) {
  LightSampleSource src;
  src.baseSample = 0;  // lightSampleID: first request2D() (pathtraceintegrator.cpp:39)
  src.sample = [lp](float ux, float uy, float* o) {
    const int w = lp->image->width, h = lp->image->height;
    float sx, sy, pdf;
    dist2d_sample(lp->ycdf, lp->ypdf, lp->xcdf, lp->xpdf, w, h, ux, uy, sx, sy, pdf);
    const float theta = kPi * sy * rcpf_(float(h));
    const float phi = kTwoPi * (1.0f - sx * rcpf_(float(w)));
    const V3 _wi = v3(-sinf(theta) * cosf(phi), cosf(theta), -sinf(theta) * sinf(phi));
    const V3 wi = xfmVector(lp->l2w, _wi);
    const float wpdf = pdf * rcpf_(kTwoPi * kPi * sinf(theta));
    float c[4];
    lp->image->get(std::max(0, std::min((int)sx, w - 1)), std::max(0, std::min((int)sy, h - 1)), c);
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = wpdf;
    o[4] = lp->L.x * c[0]; o[5] = lp->L.y * c[1]; o[6] = lp->L.z * c[2];
    o[7] = INFINITY;
  };
  return src;
}

// allLights in slot order
void SceneTables::add_lights(const Prims& prims) {
  primLight.assign(prims.size(), -1);
  for (size_t i = 0; i < prims.size(); ++i) {
    const auto& p = prims[i];
    if (!p || !p->light) continue;
    const LightInst& L = *p->light;
    GpuLight g = gpu_light_record(L);
    // EnvironmentLight subclasses (api/scene.h:76): ambient, HDRI, distant
    if (L.type == LIGHT_AMBIENT || L.type == LIGHT_HDRI || L.type == LIGHT_DISTANT) {
      g.isEnv = 1;
      // an environment light whose Le is exactly 0 for every direction (L = 0 0 0 over finite
      // texels, e.g. C4's HDRILight) only adds throughput * 0 to a missed path: k_shade leaves
      // it out and keeps the NaN such an add makes of a non-finite throughput (numEnvZero)
      bool zero = L.L.x == 0.f && L.L.y == 0.f && L.L.z == 0.f;
      if (zero && L.type == LIGHT_HDRI && L.image && L.image->format == IMG_RGBAF32) {
        const float* f = (const float*)L.image->data.data();
        for (size_t k = 0; k < L.image->data.size() / 4 && zero; ++k) zero = std::isfinite(f[k]);
      }
      if (zero) {
        ++numEnvZero;
      } else {
        envLights.push_back((int)lights.size());
        if (L.type != LIGHT_AMBIENT) ++numEnvDir;
      }
    }
    if (L.type == LIGHT_HDRI) {
      g.image = imageId(L.image);
      g.hdriW = L.image->width; g.hdriH = L.image->height;
    }
    if (L.precompute()) {
      g.precomputed = (int)precomputed.size();
      precomputed.push_back(hdri_sample_source(p->light));
    }
    primLight[i] = (int)lights.size();
    lights.push_back(g);
    allLights.push_back(p->light);
  }
}

// geometries in slot order (geomID = compacted index); after add_lights, so that a geometry can
// reference its area light
void SceneTables::add_geoms(const Prims& prims) {
  for (const auto& p : prims)
    if (p && p->shape) {
      anyMotion |= !p->shape->mot.empty();
      anyTangent |= !p->shape->tanX.empty() || !p->shape->tanY.empty();
    }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  auto push9 = [](std::vector<float>& d, V3 a, V3 b, V3 c) {
    const float t[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
    d.insert(d.end(), t, t + 9);
  };
  for (size_t i = 0; i < prims.size(); ++i) {
    const auto& p = prims[i];
    if (!p || !p->shape) continue;
    const MeshInst& m = *p->shape;
    GpuGeom g;
    memset(&g, 0, sizeof(g));
    g.kind = m.kind;
    g.material = materialId(p->material);
    g.light = primLight[i];
    g.illumMask = p->illumMask; g.shadowMask = p->shadowMask;
    g.vtxBase = (int)positions.size();
    g.triBase = numTris;
    g.flags = (m.nor.empty() ? 0 : GF_NORMALS) | (m.uv.empty() ? 0 : GF_TEXCOORDS) | (m.cull ? GF_CULL : 0) |
              (m.mot.empty() ? 0 : GF_MOTION) | (m.tanX.empty() ? 0 : GF_TANGENT_X) |
              (m.tanY.empty() ? 0 : GF_TANGENT_Y);
    g.Ng[0] = m.Ng.x; g.Ng[1] = m.Ng.y; g.Ng[2] = m.Ng.z;
    const int geomId = (int)geoms.size();
    append_f4(positions, m.pos, m.pos.size());
    append_f4(normals, m.nor, m.pos.size());
    if (anyMotion) append_f4(motions, m.mot, m.pos.size());
    for (size_t k = 0; k < m.pos.size(); ++k) {
      texcoords.push_back(m.uv.empty() ? make_float2(0.f, 0.f) : make_float2(m.uv[2 * k], m.uv[2 * k + 1]));
      if (anyTangent) {
        tangents.push_back(m.tanX.empty() ? zero : f4(m.tanX[k]));
        tangents.push_back(m.tanY.empty() ? zero : f4(m.tanY[k]));
      }
    }
    auto mot = [&](int v) { return m.mot.empty() ? v3s(0.f) : m.mot[v]; };
    const int nt = (int)(m.tri.size() / 3);
    for (int t = 0; t < nt; ++t) {
      const int a = m.tri[3 * t], b = m.tri[3 * t + 1], c = m.tri[3 * t + 2];
      indices.push_back(make_int4(g.vtxBase + a, g.vtxBase + b, g.vtxBase + c, geomId));
      triGeom.push_back(geomId);
      push9(triVerts, m.pos[a], m.pos[b], m.pos[c]);
      // p + m: the vertices at time 1 (trianglemesh_full.cpp:152-166)
      if (anyMotion) push9(triVerts1, m.pos[a] + mot(a), m.pos[b] + mot(b), m.pos[c] + mot(c));
      triFlags.push_back(m.cull ? 1u : 0u);
    }
    numTris += nt;
    geoms.push_back(g);
  }
  if (numTris >= (1 << 26)) throw std::runtime_error("scene exceeds 2^26 triangles (stack entry packing)");
}

// place the float images after the 8-bit ones; image and texture records get final offsets
void SceneTables::place_float_texels() {
  texels8Bytes = (texels.size() + 15) & ~size_t(15);
  texels.resize(texels8Bytes);
  texels.insert(texels.end(), texelsF.begin(), texelsF.end());
  for (GpuImage& g : images)
    if (g.format == IMG_RGBAF32) g.offset += (int64_t)texels8Bytes;
  for (GpuTexture& t : textures) t.offset = images[t.image].offset;
}

struct SceneBvh {
  BvhResult bvh;
  std::vector<GpuQNode> qnodes;  // the any-hit kernels' 64-B nodes (common/yrt_qnode.h), node for node
};

// Stage 2, BVH: runs the builder asked for (the host SAH builder where "morton" declines), fills S.buildInfo
static SceneBvh build_scene_bvh(GpuScene& S, const SceneTables& T, int stackDepth, bool upload, bool morton,
                                hipStream_t stream, bool timing) {
  SceneBvh B;
  BvhResult& bvh = B.bvh;
  const auto tb = std::chrono::steady_clock::now();
  const std::vector<float>* v1 = T.anyMotion ? &T.triVerts1 : nullptr;
  BuildInfo& bi = S.buildInfo;
  S.mortonAsked = morton;
  if (morton) {
    bi.builder = upload ? BUILDER_MORTON_GPU : BUILDER_MORTON_HOST;
    bi.fallback = upload ? build_bvh_morton_gpu(T.triVerts, T.triFlags, stackDepth, bvh, v1, stream, timing, &bi.msKernels)
                         : build_bvh_morton_host(T.triVerts, T.triFlags, stackDepth, bvh, v1);
  }
  if (!morton || bi.fallback != FALLBACK_NONE) {
    bi.builder = BUILDER_SAH;
    bi.msKernels = 0;
    build_bvh(T.triVerts, T.triFlags, stackDepth, bvh, v1);
  }
  bi.msBuild = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
  bi.sahCost = bvh_sah_cost(bvh.nodes);
  // each leaf record carries its triangle's geometry id (GpuTri::e2[3]): part of the record's
  // layout as exported; the kernels take the id from the shading record (GpuTriShade)
  for (size_t i = 0; i < bvh.tris.size(); ++i) memcpy(&bvh.tris[i].e2[3], &T.triGeom[bvh.order[i]], 4);
  B.qnodes.resize(bvh.nodes.size());
  for (size_t i = 0; i < bvh.nodes.size(); ++i) yrt_quantize_node(bvh.nodes[i], B.qnodes[i]);
  S.bvhDepth = bvh.maxDepth;
  return B;
}

// Stage 3, derived records. Per leaf slot: the moving triangle's other vertices and the vertex motions
static std::vector<GpuTriMotion> tri_motion_records(const SceneTables& T, const std::vector<int>& order) {
  std::vector<GpuTriMotion> tm(order.size());
  for (size_t i = 0; i < order.size(); ++i) {
    const int4 ix = T.indices[order[i]];
    GpuTriMotion& r = tm[i];
    memset(&r, 0, sizeof(r));
    st3(r.p1, T.positions[ix.y]); st3(r.p2, T.positions[ix.z]);
    st3(r.m0, T.motions[ix.x]); st3(r.m1, T.motions[ix.y]); st3(r.m2, T.motions[ix.z]);
  }
  return tm;
}

// Per triangle: what k_shade reads of its three vertices (common/yrt_tri_record.h)
static std::vector<GpuTriShade> tri_shade_records(const SceneTables& T) {
  std::vector<GpuTriShade> ts(T.indices.size());
  for (size_t t = 0; t < T.indices.size(); ++t) {
    const int4 ix = T.indices[t];
    const int v[3] = {ix.x, ix.y, ix.z};
    float p[3][3], n[3][3], st[3][2];
    for (int k = 0; k < 3; ++k) {
      st3(p[k], T.positions[v[k]]); st3(n[k], T.normals[v[k]]);
      st[k][0] = T.texcoords[v[k]].x; st[k][1] = T.texcoords[v[k]].y;
    }
    yrt_tri_shade_fill(ts[t], p[0], p[1], p[2], n[0], n[1], n[2], st[0], st[1], st[2], ix.w);
  }
  return ts;
}

// Per geometry: the geometry with its material and the material's first texture
static std::vector<GpuGeomRec> geom_records(const SceneTables& T) {
  std::vector<GpuGeomRec> recs(T.geoms.size());
  for (size_t i = 0; i < T.geoms.size(); ++i) {
    GpuGeomRec& r = recs[i];
    memset(&r, 0, sizeof(r));
    r.g = T.geoms[i];
    if (r.g.material >= 0) {
      r.m = T.materials[r.g.material];
      if (r.m.tex[0] >= 0) r.t0 = T.textures[r.m.tex[0]];
    }
  }
  return recs;
}

// Stage 4, upload and view: in this order, which is also the order of the allocations
static void upload_scene(GpuScene& S, const SceneTables& T, const SceneBvh& B) {
  for (const GpuMaterial& m : T.materials) S.materialMask |= 1u << m.type;
  for (const GpuLight& l : T.lights) S.materialMask |= 1u << (16 + l.type);  // light_bit (kernels/yrt_shade.h)
  S.nodes.upload(B.bvh.nodes);
  S.qnodes.upload(B.qnodes);
  S.tris.upload(B.bvh.tris);
  S.triGeom.upload(T.triGeom);
  S.indices.upload(T.indices);
  S.positions.upload(T.positions);
  if (T.anyMotion) {
    S.motions.upload(T.motions);
    S.triMotion.upload(tri_motion_records(T, B.bvh.order));
  }
  if (T.anyTangent) S.tangents.upload(T.tangents);
  S.normals.upload(T.normals);
  S.texcoords.upload(T.texcoords);
  S.geoms.upload(T.geoms);
  S.triShade.upload(tri_shade_records(T));
  S.geomRecs.upload(geom_records(T));
  S.materials.upload(T.materials);
  S.textures.upload(T.textures);
  S.images.upload(T.images);
  S.texels.upload(T.texels);
  S.texQuads.upload(build_tex_quads(T.images, T.texels, T.texels8Bytes));
  S.lights.upload(T.lights);
  S.envLights.upload(T.envLights);
  S.media.upload(T.media);
  bind_view(S);
}

// Stage 5, refit tables: slot -> geometry, gid -> leaf position, nodes grouped by depth (refit_gpu_scene)
static void build_refit_tables(GpuScene& S, const Prims& prims, const BvhResult& bvh, int numTris) {
  S.slotsCommitted = prims;
  S.slotGeom.assign(prims.size(), -1);
  int gcount = 0;
  for (size_t i = 0; i < prims.size(); ++i)
    if (prims[i] && prims[i]->shape) S.slotGeom[i] = gcount++;
  // gid -> leaf slots (CSR: numTris + 1 offsets, then the slots; spatial splits can put a
  // triangle in several leaves)
  std::vector<int> leafOf(numTris + 1 + bvh.order.size(), 0);
  for (int g : bvh.order) leafOf[g + 1]++;
  for (int g = 0; g < numTris; ++g) leafOf[g + 1] += leafOf[g];
  std::vector<int> fill(leafOf.begin(), leafOf.begin() + numTris);
  for (size_t i = 0; i < bvh.order.size(); ++i) leafOf[numTris + 1 + fill[bvh.order[i]]++] = (int)i;
  S.triLeaf.upload(leafOf);
  std::vector<std::vector<int>> levels;
  std::vector<std::pair<int, int>> work = {{0, 0}};
  for (size_t w = 0; w < work.size(); ++w) {
    const int ni = work[w].first, d = work[w].second;
    if ((int)levels.size() <= d) levels.resize(d + 1);
    levels[d].push_back(ni);
    for (int k = 0; k < 4; ++k) {
      const int c = bvh.nodes[ni].child[k];
      if (c != -1 && (c & 31) == 0) work.push_back({c >> 5, d + 1});
    }
  }
  std::vector<int> flat;
  S.levelStart.clear();
  for (auto& l : levels) {
    S.levelStart.push_back((int)flat.size());
    flat.insert(flat.end(), l.begin(), l.end());
  }
  S.levelStart.push_back((int)flat.size());
  S.levelNodes.upload(flat);
}

// Stage 6, counts and host mirrors: takes the tables over. The texel pool stays only with a host-only
// scene, which has no device copy of it (yrtDebugTexturePool).
static void set_mirrors(GpuScene& S, SceneTables&& T, SceneBvh&& B, bool upload) {
  S.hasMotion = T.anyMotion;
  S.numTris = S.view.numTris = T.numTris;
  S.numGeoms = (int)T.geoms.size();
  S.texels8Bytes = T.texels8Bytes; S.texelsBytes = T.texels.size();
  S.view.numNodes = (int)B.bvh.nodes.size();
  S.view.numLights = (int)T.lights.size(); S.view.numEnvLights = (int)T.envLights.size();
  S.view.numEnvZero = T.numEnvZero; S.view.numEnvDir = T.numEnvDir;
  S.hMaterials = std::move(T.materials); S.hTextures = std::move(T.textures); S.hImages = std::move(T.images);
  S.hMedia = std::move(T.media);
  if (!upload) S.hTexels = std::move(T.texels);
  S.hNodes = std::move(B.bvh.nodes); S.hQNodes = std::move(B.qnodes); S.hTris = std::move(B.bvh.tris);
  S.hGeoms = std::move(T.geoms); S.hTriGeom = std::move(T.triGeom);
  S.allLights = std::move(T.allLights); S.hLights = std::move(T.lights); S.hEnvLights = std::move(T.envLights);
  S.precomputed = std::move(T.precomputed);
}

std::shared_ptr<GpuScene> build_gpu_scene(const Prims& prims, int stackDepth, bool upload, bool morton,
                                          hipStream_t stream, bool timing) {
  auto t0 = std::chrono::steady_clock::now();
  auto S = std::make_shared<GpuScene>();
  if (upload) HIP_CHECK(hipGetDevice(&S->device));
  SceneTables T(prims);
  SceneBvh B = build_scene_bvh(*S, T, stackDepth, upload, morton, stream, timing);
  scene_bounds(prims, S->bboxLo, S->bboxHi);
  if (upload) {
    upload_scene(*S, T, B);
    build_refit_tables(*S, prims, B.bvh, T.numTris);
  }
  set_mirrors(*S, std::move(T), std::move(B), upload);
  S->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return S;
}

// The scalar fields a replica shares with its source, then the buffers of SceneBuffers::all; the
// host mirrors other than the light tables stay with the source.
std::shared_ptr<GpuScene> replicate_gpu_scene(const GpuScene& src, int device) {
  HIP_CHECK(hipSetDevice(device));
  auto R = std::make_shared<GpuScene>();
  R->device = device;
  R->serial = src.serial;  // same committed scene: the sample-table caches may key on it
  for (DevBuf SceneBuffers::*b : SceneBuffers::all) {
    const DevBuf& from = src.*b;
    if (!from.p) continue;
    ((*R).*b).alloc(from.bytes);
    HIP_CHECK(hipMemcpyPeer(((*R).*b).p, device, from.p, src.device, from.bytes));
  }
  R->hasMotion = src.hasMotion;
  R->view = src.view;
  bind_view(*R);
  R->materialMask = src.materialMask;
  R->precomputed = src.precomputed;
  R->hLights = src.hLights; R->hEnvLights = src.hEnvLights;
  R->numTris = src.numTris; R->numGeoms = src.numGeoms; R->bvhDepth = src.bvhDepth;
  R->refits = src.refits;
  R->texels8Bytes = src.texels8Bytes; R->texelsBytes = src.texelsBytes;
  return R;
}

bool refit_gpu_scene(GpuScene& S, const Prims& prims, hipStream_t stream) {
  // moving geometry: boxes span the frame time and leaf records carry motion (rebuild instead)
  if (!S.nodes.p || prims.size() != S.slotsCommitted.size() || S.hNodes.empty() || S.hasMotion) return false;
  std::vector<size_t> moved;
  for (size_t i = 0; i < prims.size(); ++i) {
    const auto& o = S.slotsCommitted[i];
    const auto& n = prims[i];
    if (o == n) continue;
    if (!o || !n || !o->shape || !n->shape || o->light || n->light) return false;
    if (o->material != n->material || o->illumMask != n->illumMask || o->shadowMask != n->shadowMask) return false;
    const MeshInst& a = *o->shape;
    const MeshInst& b = *n->shape;
    if (a.kind != b.kind || b.kind == GEOM_TRIANGLE || a.cull != b.cull) return false;
    if (a.pos.size() != b.pos.size() || a.nor.size() != b.nor.size() || a.uv != b.uv || a.tri != b.tri) return false;
    // a refit re-uploads positions and normals only: a shape that gains motion (the refit keeps
    // a static scene's boxes and flags), or whose tangents change (a moved mesh's tangents are
    // rotated with it), is rebuilt
    if (!a.mot.empty() || !b.mot.empty()) return false;
    auto same_v3 = [](const std::vector<V3>& x, const std::vector<V3>& y) {
      return x.size() == y.size() && (x.empty() || !memcmp(x.data(), y.data(), x.size() * sizeof(V3)));
    };
    if (!same_v3(a.tanX, b.tanX) || !same_v3(a.tanY, b.tanY)) return false;
    if (!same_v3(a.pos, b.pos) || !same_v3(a.nor, b.nor)) moved.push_back(i);
  }
  S.slotsCommitted = prims;  // unchanged geometry: adopt the new slot objects (export)
  if (moved.empty()) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i : moved) {
    const MeshInst& m = *prims[i]->shape;
    const GpuGeom& g = S.hGeoms[S.slotGeom[i]];
    std::vector<float4> pos, nor;
    append_f4(pos, m.pos, m.pos.size());
    append_f4(nor, m.nor, m.pos.size());
    HIP_CHECK(hipMemcpyAsync(S.positions.as<float4>() + g.vtxBase, pos.data(), pos.size() * sizeof(float4),
                             hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(S.normals.as<float4>() + g.vtxBase, nor.data(), nor.size() * sizeof(float4),
                             hipMemcpyHostToDevice, stream));
    launch_refit_tris(S.tris.as<GpuTri>(), S.triShade.as<GpuTriShade>(), S.indices.as<int4>(), S.positions.as<float4>(),
                      S.normals.as<float4>(), S.triLeaf.as<int>(), S.triLeaf.as<int>() + S.numTris + 1, g.triBase,
                      (int)(m.tri.size() / 3), stream);
    // the host copies must outlive the async copies
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  for (int d = (int)S.levelStart.size() - 2; d >= 0; --d)
    launch_refit_nodes(S.nodes.as<GpuNode>(), S.tris.as<GpuTri>(), S.indices.as<int4>(), S.positions.as<float4>(),
                       S.levelNodes.as<int>() + S.levelStart[d], S.levelStart[d + 1] - S.levelStart[d], stream);
  launch_quantize_nodes(S.nodes.as<GpuNode>(), S.qnodes.as<GpuQNode>(), (int)S.hNodes.size(), stream);
  scene_bounds(prims, S.bboxLo, S.bboxHi);  // as the build takes them
  HIP_CHECK(hipStreamSynchronize(stream));
  S.hostBvhStale = true;
  S.refits++;
  S.buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return true;
}

void sync_host_bvh(GpuScene& S) {
  if (!S.hostBvhStale) return;
  HIP_CHECK(hipMemcpy(S.hNodes.data(), S.nodes.p, S.hNodes.size() * sizeof(GpuNode), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(S.hQNodes.data(), S.qnodes.p, S.hQNodes.size() * sizeof(GpuQNode), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(S.hTris.data(), S.tris.p, S.hTris.size() * sizeof(GpuTri), hipMemcpyDeviceToHost));
  S.hostBvhStale = false;
}

}  // namespace yrt
