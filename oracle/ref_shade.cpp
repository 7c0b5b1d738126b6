// ref_shade.cpp — TEST INFRASTRUCTURE ONLY (oracle/_ref). Compiled by `make -C oracle ref` with
// clang against the reference's own, unmodified shading layer where it lies under $(REF)
// (never copied into this repo):
//   devices/device_singleray/cameras/{pinholecamera,depthoffieldcamera,StereoCubeCamera}.h
//   devices/device_singleray/brdfs/{lambertian,dielectric,dielectriclayer,microfacet,transmission,
//     specular,reflection,conductor,minnaert,velvety,compositedbrdf}.h and brdfs/microfacet/*
//   devices/device_singleray/samplers/shapesampler.h, api/parms.h
//
// Three things in this prologue are not the reference's build, and all are deliberate:
//  1. `#define final std::true_type` around the reference headers. common/math/affinespace.h:153
//     reads `struct ArrayXf : final {`, which only MSVC accepts. That primary template is
//     deleted and never instantiated, so giving it a base class changes no code that runs; it is
//     a rename of the same kind as the recipe's -D__rdtsc=... . No reference header uses `final`
//     as the C++11 specifier.
//  2. The CRT's transcendentals are SUBSTITUTED, not pinned: sinf cosf acosf asinf atanf atan2f
//     powf expf logf are defined as their yrt_* twins of csrc/common/yrt_libm.h before the
//     reference headers are read, so common/math/math.h:69-80 (sin, cos, pow, ...) calls the
//     project's shared libm. Everything *around* the transcendentals is then comparable bit for
//     bit with the oracle and the device; the functions themselves remain the unpinned boundary
//     (DESIGN.md §4). tanf (camera constructors) is the C library's on both sides.
//
// The driver's own code is glue: extern "C" entry points that build reference objects from
// plain float32/int32 arrays and call their methods over n rows. tests/test_ref_shade.py compares
// the oracle (oracle/yrt_oracle.c) and the device probe (k_check_shade) with them bit for bit.
//
// Lights: point, spot, directional, distant and triangle. The dome (AmbientLight) and HDRILight
// are left out: AmbientLight::sample asks the BackendScene for its bounds and HDRILight's
// constructor loads an image through the scene's loaders, so neither object can be made from
// plain arrays. LightSample::tMax is not returned: the integrator overwrites it before use
// (integrators/pathtraceintegrator.cpp:152).
//
// The filtered sample table goes through the reference's real SamplerFactory::init (not a
// restated call pattern).
//
// Material::shade of the nine texture-free materials is read back through the CompositedBRDF it
// fills (ref_material_components below says how). Its recorded answers
// (tests/golden/ref_shade_mat_*.npz) are compared with the oracle (tests/test_ref_shade.py) and
// with the device's own shade_material, run by the probe k_check_material on a committed scene
// (tests/test_ref_textures.py).
//
// Not built here: the textured materials, textures, postIntersect and the integrator. Textures
// and the textured materials have no live reference witness (Bilinear.h, nearestneighbor.h and
// Uber.h do not compile unmodified); tests/test_ref_textures.py pins the device and the oracle to
// an independent numpy restatement of the two texture headers and to each other, and the oracle's
// textured classes over a constant image to the untextured ones that are pinned here
// (DESIGN.md §4).
// every standard header the reference pulls in, read before `final` is renamed
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cfloat>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <emmintrin.h>
#include <immintrin.h>
#include <smmintrin.h>
#include <xmmintrin.h>

#include "../yulio-raytracer_amd/csrc/common/yrt_libm.h"

#define sinf yrt_sinf
#define cosf yrt_cosf
#define acosf yrt_acosf
#define asinf yrt_asinf
#define atanf yrt_atanf
#define atan2f yrt_atan2f
#define powf yrt_powf
#define expf yrt_expf
#define logf yrt_logf

// 3. The reference is built with MSVC, whose <cmath> declares the float overload of fabs in the
//    global namespace; libstdc++ declares it in std:: only, so that an unqualified fabs(float)
//    inside namespace embree (lights/trianglelight.h:98) would otherwise pick the C library's
//    double fabs(double), and rcp(double) = 1.0 / x after it. The overload is declared here.
inline float fabs(float x) { return __builtin_fabsf(x); }

#define final std::true_type
#include "default.h"
#include "api/parms.h"
#include "brdfs/compositedbrdf.h"
#include "brdfs/conductor.h"
#include "brdfs/dielectric.h"
#include "brdfs/dielectriclayer.h"
#include "brdfs/lambertian.h"
#include "brdfs/microfacet.h"
#include "brdfs/minnaert.h"
#include "brdfs/reflection.h"
#include "brdfs/specular.h"
#include "brdfs/transmission.h"
#include "brdfs/velvety.h"
#include "cameras/StereoCubeCamera.h"
#include "cameras/depthoffieldcamera.h"
#include "cameras/pinholecamera.h"
// The light constructors call cosf by name (spotlight.h:29-30, distantlight.h:29): a value made
// once per light on the host, with the C library's cosf on the oracle's and the device's side
// too. They are read without the cosf substitution; the samplers' cos() / sin() go through
// common/math/math.h, which is already read, and stay substituted.
#undef cosf
#include "samplers/sampler.h"
#include "lights/directionallight.h"
#include "lights/distantlight.h"
#include "lights/pointlight.h"
#include "lights/spotlight.h"
#include "lights/trianglelight.h"
#include "materials/brushedmetal.h"
#include "materials/dielectric.h"
#include "materials/matte.h"
#include "materials/metal.h"
#include "materials/metallicpaint.h"
#include "materials/mirror.h"
#include "materials/plastic.h"
#include "materials/thindielectric.h"
#include "materials/velvet.h"
// the sampler, its distributions and the pixel filter, as translation units of this library
#include "filters/bsplinefilter.h"
#include "filters/filter.cpp"
#include "samplers/distribution1d.cpp"
#include "samplers/distribution2d.cpp"
#include "samplers/sampler.cpp"
#undef final

using namespace embree;

// TriangleLight owns a Triangle shape (lights/trianglelight.h:49), whose extract() hands the
// triangle to Embree. Nothing here builds a scene, so these three are never called; they exist so
// that the library links without Embree's binary (-Wl,-z,defs) and stop the process if reached.
extern "C" unsigned rtcNewTriangleMesh(RTCScene, RTCGeometryFlags, size_t, size_t, size_t) { abort(); }
extern "C" void* rtcMapBuffer(RTCScene, unsigned, RTCBufferType) { abort(); }
extern "C" void rtcUnmapBuffer(RTCScene, unsigned, RTCBufferType) { abort(); }

namespace {

// ---- cameras: params[32] (tests/ref_shade_cases.py CAM_FIELDS); bit i of params[31] = field i
// is present in the Parms (absent ones take the class's defaults)
enum { CF_L2W, CF_ANGLE, CF_ASPECT, CF_LENS, CF_FOCAL, CF_FACE, CF_TOEIN, CF_EYESEP, CF_ZPD, CF_FALLOFF, CF_SCALE,
       CF_ORIGIN, CF_LOOKAT, CF_UP };

Parms camera_parms(const float* p) {
  const unsigned mask = (unsigned)p[31];
  auto has = [&](int f) { return (mask >> f) & 1u; };
  Parms P;
  if (has(CF_L2W))
    P.add("local2world", Variant(AffineSpace3f(Vector3f(p[0], p[1], p[2]), Vector3f(p[3], p[4], p[5]),
                                               Vector3f(p[6], p[7], p[8]), Vector3f(p[9], p[10], p[11]))));
  if (has(CF_ANGLE)) P.add("angle", Variant(p[12]));
  if (has(CF_ASPECT)) P.add("aspectRatio", Variant(p[13]));
  if (has(CF_LENS)) P.add("lensRadius", Variant(p[14]));
  if (has(CF_FOCAL)) P.add("focalDistance", Variant(p[15]));
  if (has(CF_FACE)) P.add("cubeFaceIndex", Variant((int)p[16]));
  if (has(CF_TOEIN)) P.add("toeIn", Variant(p[17] != 0.f));
  if (has(CF_EYESEP)) P.add("eyeSeparation", Variant(p[18]));
  if (has(CF_ZPD)) P.add("zeroParallaxDistance", Variant(p[19]));
  if (has(CF_FALLOFF)) P.add("stereFalloffAngle", Variant(p[20]));
  if (has(CF_SCALE)) P.add("sceneScale", Variant(p[21]));
  if (has(CF_ORIGIN)) P.add("origin", Variant(p[22], p[23], p[24]));
  if (has(CF_LOOKAT)) P.add("lookAt", Variant(p[25], p[26], p[27]));
  if (has(CF_UP)) P.add("up", Variant(p[28], p[29], p[30]));
  return P;
}

// ---- BRDF components: params[16] = R.rgb, p0, p1, p2, eta.rgb, k.rgb, pad (the constructor
// arguments of the class named in kernels/yrt_shade.h's CompKind comments)
typedef Microfacet<FresnelDielectric, PowerCosineDistribution> MicroDiel;
typedef Microfacet<FresnelConductor, PowerCosineDistribution> MicroCond;
typedef Microfacet<FresnelConductor, AnisotropicPowerCosineDistribution> MicroAniso;

Color col3(const float* p) { return Color(p[0], p[1], p[2]); }

// placement-new into `buf` (64-byte aligned, as CompositedBRDF::alloc hands out)
const BRDF* make_brdf(int kind, const float* p, const DifferentialGeometry& dg, void* buf) {
  const Color R = col3(p), eta = col3(p + 6), k = col3(p + 9);
  switch (kind) {
    case 0: return new (buf) Lambertian(R);
    case 1: return new (buf) DielectricReflection(p[3], p[4], p[5]);
    case 2: return new (buf) ConstDielectricTransmission(p[3]);
    case 3: return new (buf) ThinDielectricTransmission(p[3], p[4], R, p[5]);
    case 4: return new (buf) DielectricLayer<Lambertian>(one, p[3], p[4], Lambertian(R));
    case 5: return new (buf) MicroDiel(R, FresnelDielectric(p[3], p[4]), PowerCosineDistribution(p[5], dg.Ns));
    case 6: return new (buf) Transmission(R);
    case 7: return new (buf) Specular(R, p[3]);
    case 8: return new (buf) Reflection(R);
    case 9: return new (buf) Conductor(R, eta, k);
    case 10: return new (buf) MicroCond(R, FresnelConductor(eta, k), PowerCosineDistribution(p[3], dg.Ns));
    case 11:
      return new (buf)
          MicroAniso(R, FresnelConductor(eta, k), AnisotropicPowerCosineDistribution(dg.Tx, p[3], dg.Ty, p[4], dg.Ns));
    case 12: return new (buf) Minnaert(R, p[3]);
    case 13: return new (buf) Velvety(R, p[3]);
    case 14: return new (buf) DielectricTransmission(p[3], p[4]);
    case 15:  // MetallicPaint's glitter (materials/metallicpaint.h:63-70): aluminium flakes
      return new (buf) DielectricLayer<MicroCond>(
          one, p[3], p[4],
          MicroCond(R, FresnelConductor(Color(0.62f), Color(4.8f)), PowerCosineDistribution(p[5], dg.Ns)));
  }
  return nullptr;
}

Vector3f vec3(const float* p) { return Vector3f(p[0], p[1], p[2]); }
void put3(float* o, const Vector3f& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
void putc(float* o, const Color& c) { o[0] = c.r; o[1] = c.g; o[2] = c.b; }

void fill_dg(DifferentialGeometry& dg, const float* Ns, const float* Ng, const float* Tx, const float* Ty) {
  dg.P = Vector3f(zero);
  dg.Ns = vec3(Ns);
  dg.Ng = vec3(Ng);
  dg.Tx = vec3(Tx);
  dg.Ty = vec3(Ty);
  dg.st = Vec2f(0.f, 0.f);
  dg.error = 0.f;
}

struct __align(64) Slot { char b[1024]; };

}  // namespace

extern "C" {

// kind 0 PinHoleCamera, 1 DepthOfFieldCamera, 2 StereoCubeCamera; pixel, lens: n x 2; org, dir: n x 3
int ref_camera_rays(int kind, const float* params, int n, const float* pixel, const float* lens, float* org,
                    float* dir) {
  const Parms P = camera_parms(params);
  Ref<Camera> cam;
  if (kind == 0) cam = new PinHoleCamera(P);
  else if (kind == 1) cam = new DepthOfFieldCamera(P);
  else if (kind == 2) cam = new StereoCubeCamera(P);
  else return -1;
  for (int i = 0; i < n; ++i) {
    Ray r;
    cam->ray(Vec2f(pixel[2 * i], pixel[2 * i + 1]), Vec2f(lens[2 * i], lens[2 * i + 1]), r);
    put3(org + 3 * i, r.org);
    put3(dir + 3 * i, r.dir);
  }
  return 0;
}

// BRDF::eval at wi and BRDF::sample at s of one component per row. params n x 16; wo, Ns, Ng, Tx,
// Ty, wi n x 3; s n x 2; out: eval3, sample3, wi_out3 n x 3, pdf n. The Sample3f handed to
// sample() starts as (zero, 0): components that return early leave it untouched.
int ref_brdf(int kind, const float* params, int n, const float* wo, const float* Ns, const float* Ng, const float* Tx,
             const float* Ty, const float* wi, const float* s, float* eval3, float* sample3, float* wi_out3,
             float* pdf) {
  Slot slot;
  for (int i = 0; i < n; ++i) {
    DifferentialGeometry dg;
    fill_dg(dg, Ns + 3 * i, Ng + 3 * i, Tx + 3 * i, Ty + 3 * i);
    const BRDF* b = make_brdf(kind, params + 16 * i, dg, &slot);
    if (!b) return -1;
    const Vector3f o = vec3(wo + 3 * i);
    putc(eval3 + 3 * i, b->eval(o, dg, vec3(wi + 3 * i)));
    Sample3f w(Vector3f(zero), 0.0f);
    putc(sample3 + 3 * i, b->sample(o, dg, w, Vec2f(s[2 * i], s[2 * i + 1])));
    put3(wi_out3 + 3 * i, w.value);
    pdf[i] = w.pdf;
    b->~BRDF();
  }
  return 0;
}

// CompositedBRDF::sample (brdfs/compositedbrdf.h:104-166) over nk <= 3 components per row, added
// in the order of kinds[]. params n x nk x 16; frame n x 12 = Ns, Ng, Tx, Ty; s n x 2; ss n.
int ref_brdf_set_sample(int nk, const int32_t* kinds, const float* params, int n, const float* wo, const float* frame,
                        const float* s, const float* ss, float* color3, float* wi3, float* pdf, uint32_t* type) {
  if (nk < 1 || nk > 3) return -1;
  Slot slot[3];
  alignas(64) static thread_local char setbuf[sizeof(CompositedBRDF)];
  for (int i = 0; i < n; ++i) {
    DifferentialGeometry dg;
    const float* f = frame + 12 * i;
    fill_dg(dg, f, f + 3, f + 6, f + 9);
    CompositedBRDF* set = new (setbuf) CompositedBRDF;
    const BRDF* b[3];
    for (int k = 0; k < nk; ++k) {
      b[k] = make_brdf(kinds[k], params + ((size_t)i * nk + k) * 16, dg, &slot[k]);
      if (!b[k]) return -1;
      set->add(b[k]);
    }
    Sample3f w(Vector3f(zero), 0.0f);
    BRDFType t = (BRDFType)0;
    size_t index = 0;
    putc(color3 + 3 * i, set->sample(vec3(wo + 3 * i), dg, w, t, index, Vec2f(s[2 * i], s[2 * i + 1]), ss[i]));
    put3(wi3 + 3 * i, w.value);
    pdf[i] = w.pdf;
    type[i] = (uint32_t)t;
    for (int k = 0; k < nk; ++k) b[k]->~BRDF();
    set->~CompositedBRDF();
  }
  return 0;
}

// Light::sample after Light::transform(xfm): kind as the device's LightType (1 triangle, 3 point,
// 4 spot, 5 directional, 6 distant). params[32] = xfm (vx, vy, vz, p), a.xyz (P | v0), b.xyz (D |
// v1), c.xyz (v2), colour (I | E | L), f0 (angleMin | halfAngle, degrees), f1 (angleMax).
// P n x 3 shade points, s n x 2; out L3, wi3 n x 3, pdf n. The LightSample starts as (zero, 0).
int ref_light_sample(int kind, const float* p, int n, const float* P, const float* s, float* L3, float* wi3,
                     float* pdf) {
  Parms parms;
  const AffineSpace3f xfm(Vector3f(p[0], p[1], p[2]), Vector3f(p[3], p[4], p[5]), Vector3f(p[6], p[7], p[8]),
                          Vector3f(p[9], p[10], p[11]));
  Ref<Light> base;
  if (kind == 1) {
    parms.add("v0", Variant(p[12], p[13], p[14]));
    parms.add("v1", Variant(p[15], p[16], p[17]));
    parms.add("v2", Variant(p[18], p[19], p[20]));
    parms.add("L", Variant(p[21], p[22], p[23]));
    base = new TriangleLight(parms);
  } else if (kind == 3) {
    parms.add("P", Variant(p[12], p[13], p[14]));
    parms.add("I", Variant(p[21], p[22], p[23]));
    base = new PointLight(parms);
  } else if (kind == 4) {
    parms.add("P", Variant(p[12], p[13], p[14]));
    parms.add("D", Variant(p[15], p[16], p[17]));
    parms.add("I", Variant(p[21], p[22], p[23]));
    parms.add("angleMin", Variant(p[24]));
    parms.add("angleMax", Variant(p[25]));
    base = new SpotLight(parms);
  } else if (kind == 5) {
    parms.add("D", Variant(p[15], p[16], p[17]));
    parms.add("E", Variant(p[21], p[22], p[23]));
    base = new DirectionalLight(parms);
  } else if (kind == 6) {
    parms.add("D", Variant(p[15], p[16], p[17]));
    parms.add("L", Variant(p[21], p[22], p[23]));
    parms.add("halfAngle", Variant(p[24]));
    base = new DistantLight(parms);
  } else {
    return -1;
  }
  Ref<Light> light = base->transform(xfm, -1, -1);
  for (int i = 0; i < n; ++i) {
    DifferentialGeometry dg;
    const float z[3] = {0.f, 0.f, 1.f}, x[3] = {1.f, 0.f, 0.f}, y[3] = {0.f, 1.f, 0.f};
    fill_dg(dg, z, z, x, y);
    dg.P = vec3(P + 3 * i);
    LightSample ls;
    ls.wi = Sample3f(Vector3f(zero), 0.0f);
    putc(L3 + 3 * i, light->sample(dg, ls, Vec2f(s[2 * i], s[2 * i + 1])));
    put3(wi3 + 3 * i, ls.wi.value);
    pdf[i] = ls.wi.pdf;
  }
  return 0;
}

// The sample table with the B-spline pixel filter, through the reference's REAL
// SamplerFactory::init (samplers/sampler.cpp:85-158; it needs no renderer: constructor, request1D,
// request2D, init with a BSplineFilter) and its own Distribution2D / filter.cpp. filter 0: none,
// 1: bspline. out[dim][set * spp + s], dims pixel.xy, lens.xy, time, 1D[n1], 2D[n2] (x, y): the
// layout of ref_kat.cpp's ref_sample_table_nofilter. Returns the record count.
int ref_sample_table(int spp, int sets, int iteration, int n1, int n2, int filter, float* out) {
  Ref<SamplerFactory> f = new SamplerFactory((unsigned)spp, (unsigned)sets);
  f->request1D(n1);
  f->request2D(n2);
  Ref<Filter> flt = filter ? new BSplineFilter : nullptr;
  f->init(iteration, flt);
  const int rec = f->sampleSets * f->samplesPerPixel;
  auto T = [&](int d, int rc) -> float& { return out[(size_t)d * rec + rc]; };
  for (int set = 0; set < f->sampleSets; set++)
    for (int s = 0; s < f->samplesPerPixel; s++) {
      const PrecomputedSample& p = f->samples[set][s];
      const int rc = set * f->samplesPerPixel + s;
      T(0, rc) = p.pixel.x; T(1, rc) = p.pixel.y;
      T(2, rc) = p.lens.x; T(3, rc) = p.lens.y;
      T(4, rc) = p.time;
      for (int d = 0; d < n1; d++) T(5 + d, rc) = p.samples1D[d];
      for (int d = 0; d < n2; d++) {
        T(5 + n1 + 2 * d, rc) = p.samples2D[d].x;
        T(5 + n1 + 2 * d + 1, rc) = p.samples2D[d].y;
      }
    }
  return rec;
}

// Material::shade of a texture-free material built from Parms, read back through the
// CompositedBRDF it fills: the number of components, and per component its type flags and its own
// eval at wi and sample at s on the row's directions (the component classes keep their members
// private; what a component was built with shows in what it returns, and the components
// themselves are pinned by ref_brdf). type: the material's class name; its Parms are nparm entries
// (names[i], sizes[i] = 1 float or 3, values[4 i ..]). medium[4] = the current medium's
// transmission and eta (Dielectric picks its side by it). rows n x 20 = wo, Ns, Ng, Tx, Ty, wi
// (3 each), s.xy; out n x 34 = count, then 3 x (type, eval3, sample3, wi3, pdf).
int ref_material_components(const char* type, int nparm, const char* const* names, const int32_t* sizes,
                            const float* values, const float* medium, int n, const float* rows, float* out) {
  Parms P;
  for (int i = 0; i < nparm; ++i) {
    const float* v = values + 4 * i;
    if (sizes[i] == 3) P.add(names[i], Variant(v[0], v[1], v[2]));
    else P.add(names[i], Variant(v[0]));
  }
  const std::string t(type);
  Ref<Material> m;
  if (t == "Matte") m = new Matte(P);
  else if (t == "MetallicPaint") m = new MetallicPaint(P);
  else if (t == "ThinDielectric") m = new ThinDielectric(P);
  else if (t == "Plastic") m = new Plastic(P);
  else if (t == "Dielectric") m = new Dielectric(P);
  else if (t == "Mirror") m = new Mirror(P);
  else if (t == "Metal") m = new Metal(P);
  else if (t == "BrushedMetal") m = new BrushedMetal(P);
  else if (t == "Velvet") m = new Velvet(P);
  else return -1;
  const Medium cur(Color(medium[0], medium[1], medium[2]), medium[3]);
  alignas(64) static thread_local char setbuf[sizeof(CompositedBRDF)];
  for (int i = 0; i < n; ++i) {
    const float* r = rows + 20 * i;
    float* o = out + 34 * i;
    memset(o, 0, 34 * sizeof(float));
    DifferentialGeometry dg;
    fill_dg(dg, r + 3, r + 6, r + 9, r + 12);
    const Vector3f wo = vec3(r);
    CompositedBRDF* set = new (setbuf) CompositedBRDF;
    m->shade(Ray(Vector3f(zero), -wo), cur, dg, *set);
    if (set->size() > 3) return -2;
    const int32_t count = (int32_t)set->size();
    memcpy(o, &count, 4);
    for (size_t k = 0; k < set->size(); ++k) {
      const BRDF* b = (*set)[k];
      float* c = o + 1 + 11 * k;
      const uint32_t ty = (uint32_t)b->type;
      memcpy(c, &ty, 4);
      putc(c + 1, b->eval(wo, dg, vec3(r + 15)));
      Sample3f w(Vector3f(zero), 0.0f);
      putc(c + 4, b->sample(wo, dg, w, Vec2f(r[18], r[19])));
      put3(c + 7, w.value);
      c[10] = w.pdf;
    }
    set->~CompositedBRDF();
  }
  return 0;
}

}  // extern "C"
