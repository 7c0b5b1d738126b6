// api_objects.cpp — the C-ABI entry points (include/yrt_device.h) of the reference's Device
// virtuals: device and object creation, properties, commit, render, framebuffer map, ray queries,
// and the denoise stage. Reference counterpart: SingleRayDevice
// (device_singleray/api/singleray_device.cpp:99-709).
#include <strings.h>

#include "../common/yrt_cube_tap.h"
#include "../common/yrt_pixel_variance.h"
#include "device.h"
#include "image_io.h"

using namespace yrt;

extern "C" {

// parms: "" or "device=<k>" (one HIP device), "devices=<a,b,...>" or "devices=all" (tiles dealt
// over several; a device id may repeat: logical shards on one GPU), "host" (no GPU: loaders,
// BVH and frame export only, for CPU tests)
YRTDevice yrtNewDevice(const char* parms, size_t, int, const char*) {
  std::vector<int> devs = {0};
  bool gpu = true;
  try {
    if (parms && strncmp(parms, "device=", 7) == 0) devs = {atoi(parms + 7)};
    if (parms && strncmp(parms, "devices=", 8) == 0) {
      devs.clear();
      if (!strcmp(parms + 8, "all")) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return nullptr;
        for (int k = 0; k < n; ++k) devs.push_back(k);
      } else {
        for (const char* p = parms + 8; *p;) {
          devs.push_back(atoi(p));
          while (*p && *p != ',') ++p;
          if (*p == ',') ++p;
        }
      }
      if (devs.empty()) return nullptr;
    }
    if (parms && strcmp(parms, "host") == 0) gpu = false;
    auto* d = new YRTDevice_;
    d->d = new Device(devs, gpu);
    return d;
  } catch (...) {
    return nullptr;
  }
}

void yrtDeleteDevice(YRTDevice dev) {
  if (!dev) return;
  delete dev->d;
  delete dev;
}

const char* yrtGetLastError(YRTDevice dev) { return dev && dev->d ? dev->d->lastError.c_str() : "no device"; }

static bool ieq(const char* a, const char* b) { return a && b && strcasecmp(a, b) == 0; }

YRTHandle yrtNewCamera(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  if (!ieq(type, "pinhole") && !ieq(type, "depthoffield") && !ieq(type, "stereo"))
    throw std::runtime_error(std::string("unknown camera type: ") + type);
  return dev->d->wrap(std::make_shared<CameraObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewData(YRTDevice dev, const char* type, size_t bytes, const void* data) {
  DEV_GUARD(dev, nullptr)
  auto o = std::make_shared<DataObj>();
  o->type = type ? type : "immutable";
  o->bytes.assign((const uint8_t*)data, (const uint8_t*)data + bytes);
  return dev->d->wrap(o);
  DEV_END(nullptr)
}

// SingleRayDevice::rtNewDataFromFile (singleray_device.cpp:204-222)
YRTHandle yrtNewDataFromFile(YRTDevice dev, const char* type, const char* file, size_t offset, size_t bytes) {
  DEV_GUARD(dev, nullptr)
  if (!file) throw std::runtime_error("invalid file name");
  if (!strncmp(file, "server:", 7)) file += 7;
  if (strcasecmp(type, "immutable") != 0) throw std::runtime_error(std::string("unknown data buffer type: ") + type);
  FILE* f = fopen(file, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open file ") + file);
  auto d = std::make_shared<DataObj>();
  d->bytes.resize(bytes);
  fseek(f, (long)offset, SEEK_SET);
  const size_t got = fread(d->bytes.data(), 1, bytes, f);
  fclose(f);
  if (got != bytes) throw std::runtime_error("error filling data buffer from file");
  return dev->d->wrap(d);
  DEV_END(nullptr)
}

YRTHandle yrtNewImage(YRTDevice dev, const char* type, size_t width, size_t height, const void* data) {
  DEV_GUARD(dev, nullptr)
  auto o = std::make_shared<ImageObj>();
  image_from_memory(type, (int)width, (int)height, data, *o);
  return dev->d->wrap(o);
  DEV_END(nullptr)
}

YRTHandle yrtNewImageFromFile(YRTDevice dev, const char* file) {
  DEV_GUARD(dev, nullptr)
  auto o = std::make_shared<ImageObj>();
  // SingleRayDevice::rtNewImageFromFile (singleray_device.cpp:238-251): failed load -> 1x1 white
  if (!image_load(file, *o)) {
    o->width = o->height = 1;
    o->format = IMG_RGBA8;
    o->data = {255, 255, 255, 255};
  }
  return dev->d->wrap(o);
  DEV_END(nullptr)
}

YRTHandle yrtNewTexture(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  if (!ieq(type, "bilinear") && !ieq(type, "nearest") && !ieq(type, "image"))
    throw std::runtime_error(std::string("unsupported texture type: ") + type);
  return dev->d->wrap(std::make_shared<TextureObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewMaterial(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  // SingleRayDevice::rtNewMaterial (api/singleray_device.cpp:262-280)
  static const char* ok[] = {"Matte", "Plastic", "Dielectric", "Glass", "ThinDielectric", "ThinGlass", "Mirror",
                             "Metal", "BrushedMetal", "MetallicPaint", "MatteTextured", "Uber", "Obj", "Velvet"};
  bool found = false;
  for (auto* n : ok) found |= ieq(type, n);
  if (!found) throw std::runtime_error(std::string("unknown material type: ") + type);
  return dev->d->wrap(std::make_shared<MaterialObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewShape(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  if (!ieq(type, "trianglemesh") && !ieq(type, "sphere") && !ieq(type, "triangle") && !ieq(type, "disk"))
    throw std::runtime_error(std::string("shape type '") + type + "' is outside the MI355X device's scope");
  return dev->d->wrap(std::make_shared<ShapeObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewLight(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  // SingleRayDevice::rtNewLight (api/singleray_device.cpp:293-302)
  static const char* ok[] = {"ambientlight", "pointlight", "spotlight", "directionallight", "distantlight",
                             "hdrilight", "trianglelight"};
  bool found = false;
  for (auto* n : ok) found |= ieq(type, n);
  if (!found) throw std::runtime_error(std::string("unknown light type: ") + type);
  return dev->d->wrap(std::make_shared<LightObj>(type));
  DEV_END(nullptr)
}

static A3 xfm_or_identity(const float* t) {
  if (!t) return a3_identity();
  return a3(l3(v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8])), v3(t[9], t[10], t[11]));
}

YRTHandle yrtNewShapePrimitive(YRTDevice dev, YRTHandle shape, YRTHandle material, const float* transform12,
                               int faceCamera) {
  DEV_GUARD(dev, nullptr)
  auto p = std::make_shared<PrimitiveObj>();
  p->shapeHandle = dev->d->get<ShapeObj>(shape, "shape");
  p->materialHandle = dev->d->get<MaterialObj>(material, "material");
  if (!p->shapeHandle) throw std::runtime_error("invalid shape handle");
  p->transform = xfm_or_identity(transform12);
  p->faceCamera = faceCamera != 0;
  return dev->d->wrap(p);
  DEV_END(nullptr)
}

YRTHandle yrtNewLightPrimitive(YRTDevice dev, YRTHandle light, YRTHandle material, const float* transform12) {
  DEV_GUARD(dev, nullptr)
  auto p = std::make_shared<PrimitiveObj>();
  p->lightHandle = dev->d->get<LightObj>(light, "light");
  p->materialHandle = dev->d->get<MaterialObj>(material, "material");
  if (!p->lightHandle) throw std::runtime_error("invalid light handle");
  p->transform = xfm_or_identity(transform12);
  return dev->d->wrap(p);
  DEV_END(nullptr)
}

// SingleRayDevice::rtTransformPrimitive (singleray_device.cpp:328-334) ->
// PrimitiveHandle(space, other): transform = space * other.transform (api/instance.h:47-51)
YRTHandle yrtTransformPrimitive(YRTDevice dev, YRTHandle prim, const float* transform12) {
  DEV_GUARD(dev, nullptr)
  auto o = dev->d->get<PrimitiveObj>(prim, "primitive");
  if (!o) throw std::runtime_error("invalid primitive handle");
  auto p = std::make_shared<PrimitiveObj>(*o);
  p->transform = mul(xfm_or_identity(transform12), o->transform);
  return dev->d->wrap(p);
  DEV_END(nullptr)
}

YRTHandle yrtNewScene(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  return dev->d->wrap(std::make_shared<SceneObj>(type ? type : "default"));
  DEV_END(nullptr)
}

// BackendSceneFlat::Handle::setPrimitive (api/scene_flat.h:48-58)
int yrtSetPrimitive(YRTDevice dev, YRTHandle scene, size_t slot, YRTHandle prim) {
  DEV_GUARD(dev, -1)
  auto s = dev->d->get<SceneObj>(scene, "scene");
  auto p = dev->d->get<PrimitiveObj>(prim, "primitive");
  if (!s || !p) throw std::runtime_error("invalid scene or primitive");
  if (slot >= s->slots.size()) s->slots.resize(slot + 1);
  auto sp = std::make_shared<ScenePrim>();
  std::shared_ptr<const MeshInst> shape;
  std::shared_ptr<const LightInst> light;
  if (p->shapeHandle) {
    if (!p->shapeHandle->inst) throw std::runtime_error("shape not committed");
    shape = p->shapeHandle->inst;
  }
  if (p->lightHandle) {
    if (!p->lightHandle->inst) throw std::runtime_error("light not committed");
    light = p->lightHandle->inst;
    shape = light->shape;
  }
  if (shape) sp->shape = shape->transform(p->transform);
  if (light) sp->light = light->transform(p->transform, p->illumMask, p->shadowMask);
  if (p->materialHandle) {
    if (!p->materialHandle->inst) throw std::runtime_error("material not committed");
    sp->material = p->materialHandle->inst;
  }
  sp->illumMask = p->illumMask;
  sp->shadowMask = p->shadowMask;
  sp->faceCamera = p->faceCamera;
  sp->prim = p;
  s->slots[slot] = sp;
  return 0;
  DEV_END(-1)
}

// SingleRayDevice::rtUpdatePrimitive (singleray_device.cpp:354-398): re-orients a faceCamera
// primitive toward the camera position projected on the floor and replaces the scene slot
// (BackendSceneFlat::Handle::updatePrimitive, api/scene_flat.h:75-85). The caller re-commits
// the scene (renderer.cpp:550-559).
int yrtUpdatePrimitive(YRTDevice dev, YRTHandle scene, size_t slot, YRTHandle prim, const float* camPos3,
                       const float* camUp3) {
  DEV_GUARD(dev, -1)
  auto s = dev->d->get<SceneObj>(scene, "scene");
  if (!s) throw std::runtime_error("invalid scene handle");
  if (!prim) {
    if (slot < s->slots.size()) s->slots[slot].reset();
    return 0;
  }
  auto p = dev->d->get<PrimitiveObj>(prim, "primitive");
  if (!p->faceCamera) return 0;
  const V3 camPos = v3(camPos3[0], camPos3[1], camPos3[2]);
  const V3 camUp = v3(camUp3[0], camUp3[1], camUp3[2]);
  const V3 primPos = p->transform.p;
  V3 toEye = camPos - primPos;
  toEye.y = 0.f;
  toEye = normalize(toEye);
  const A3 lookAt = lookAtPoint(v3s(0.f), toEye, camUp);
  V3 right = cross(camUp, v3(0.f, 0.f, 1.f));
  if (right.x == 0.f && right.y == 0.f && right.z == 0.f) right = cross(camUp, v3(0.f, 1.f, 0.f));
  if (right.x == 0.f && right.y == 0.f && right.z == 0.f) right = cross(camUp, v3(1.f, 0.f, 0.f));
  const A3 makeVertical = a3_rotate_about(v3s(0.f), right, deg2rad(-90.f));
  A3 xf = mul(mul(a3_translate(primPos), lookAt), makeVertical);
  // glm::decompose scale: column lengths, negated when the linear part flips orientation
  const L3& l = p->transform.l;
  V3 sc = v3(length(l.vx), length(l.vy), length(l.vz));
  if (dot(l.vx, cross(l.vy, l.vz)) < 0.f) sc = -sc;
  if (sc.x != 0.f && sc.y != 0.f && sc.z != 0.f) xf = mul(xf, a3_scale(sc));
  if (slot > s->slots.size()) return 0;
  if (slot == s->slots.size()) s->slots.resize(slot + 1);
  auto sp = std::make_shared<ScenePrim>();
  std::shared_ptr<const MeshInst> shape;
  std::shared_ptr<const LightInst> light;
  if (p->shapeHandle && p->shapeHandle->inst) shape = p->shapeHandle->inst;
  if (p->lightHandle && p->lightHandle->inst) {
    light = p->lightHandle->inst;
    shape = light->shape;
  }
  if (shape) sp->shape = shape->transform(xf);
  if (light) sp->light = light->transform(xf, p->illumMask, p->shadowMask);
  if (p->materialHandle) sp->material = p->materialHandle->inst;
  sp->illumMask = p->illumMask;
  sp->shadowMask = p->shadowMask;
  sp->faceCamera = true;
  auto exportPrim = std::make_shared<PrimitiveObj>(*p);
  exportPrim->transform = xf;  // the frame blob carries the applied transform
  exportPrim->faceCamera = false;
  sp->prim = exportPrim;
  s->slots[slot] = sp;
  return 0;
  DEV_END(-1)
}

YRTHandle yrtNewToneMapper(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  if (!ieq(type, "default")) throw std::runtime_error(std::string("unknown tonemapper: ") + type);
  return dev->d->wrap(std::make_shared<ToneMapperObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewRenderer(YRTDevice dev, const char* type) {
  DEV_GUARD(dev, nullptr)
  if (!ieq(type, "pathtracer") && !ieq(type, "pt") && !ieq(type, "debug") && !ieq(type, "integrator"))
    throw std::runtime_error(std::string("unknown renderer: ") + type);
  return dev->d->wrap(std::make_shared<RendererObj>(type));
  DEV_END(nullptr)
}

YRTHandle yrtNewFrameBuffer(YRTDevice dev, const char* type, size_t width, size_t height, size_t buffers, void** ptrs) {
  DEV_GUARD(dev, nullptr)
  auto f = std::make_shared<FrameBufferObj>(type);
  if (ieq(type, "RGB8")) { f->format = FB_RGB8; f->stride = rgb8_row_stride(width); }
  else if (ieq(type, "RGBA8")) { f->format = FB_RGBA8; f->stride = 4 * width; }
  else if (ieq(type, "RGB_FLOAT32")) { f->format = FB_RGB_FLOAT32; f->stride = 12 * width; }
  else if (ieq(type, "RGBA_FLOAT32")) { f->format = FB_RGBA_FLOAT32; f->stride = 16 * width; }
  else throw std::runtime_error(std::string("unknown framebuffer format: ") + type);
  f->width = (int)width;
  f->height = (int)height;
  f->depth = (int)std::max<size_t>(1, buffers);
  if (ptrs) f->userPtrs.assign(ptrs, ptrs + f->depth);
  else
    for (int i = 0; i < f->depth; ++i) f->host.emplace_back(new HostPixels(f->stride * height, dev->d->gpu));
  return dev->d->wrap(f);
  DEV_END(nullptr)
}

int yrtIncRef(YRTDevice dev, YRTHandle h) {
  DEV_GUARD(dev, -1)
  dev->d->ref(h)->refs++;
  return 0;
  DEV_END(-1)
}

int yrtDecRef(YRTDevice dev, YRTHandle h) {
  DEV_GUARD(dev, -1)
  HandleRef* r = dev->d->ref(h);
  if (--r->refs == 0) {
    dev->d->handles.erase(r);
    delete r;
  }
  return 0;
  DEV_END(-1)
}

static int set_variant(YRTDevice dev, YRTHandle h, const char* prop, const Variant& v) {
  DEV_GUARD(dev, -1)
  if (!prop) throw std::runtime_error("invalid property");
  auto& obj = dev->d->ref(h)->obj;
  obj->parms.set(prop, v);
  // PrimitiveHandle::set applies immediately (api/instance.h:54-60)
  if (auto p = std::dynamic_pointer_cast<PrimitiveObj>(obj)) {
    if (!strcmp(prop, "illumMask")) p->illumMask = v.i[0];
    else if (!strcmp(prop, "shadowMask")) p->shadowMask = v.i[0];
    else if (!strcmp(prop, "faceCamera")) p->faceCamera = v.i[0] != 0;
  }
  return 0;
  DEV_END(-1)
}

int yrtSetBool1(YRTDevice dev, YRTHandle h, const char* p, int x) {
  Variant v; v.type = Variant::BOOL1; v.i[0] = x != 0;
  return set_variant(dev, h, p, v);
}
int yrtSetBool2(YRTDevice dev, YRTHandle h, const char* p, int x, int y) {
  Variant v; v.type = Variant::BOOL2; v.i[0] = x != 0; v.i[1] = y != 0;
  return set_variant(dev, h, p, v);
}
int yrtSetBool3(YRTDevice dev, YRTHandle h, const char* p, int x, int y, int z) {
  Variant v; v.type = Variant::BOOL3; v.i[0] = x != 0; v.i[1] = y != 0; v.i[2] = z != 0;
  return set_variant(dev, h, p, v);
}
int yrtSetBool4(YRTDevice dev, YRTHandle h, const char* p, int x, int y, int z, int w) {
  Variant v; v.type = Variant::BOOL4; v.i[0] = x != 0; v.i[1] = y != 0; v.i[2] = z != 0; v.i[3] = w != 0;
  return set_variant(dev, h, p, v);
}
int yrtSetInt1(YRTDevice dev, YRTHandle h, const char* p, int x) {
  Variant v; v.type = Variant::INT1; v.i[0] = x;
  return set_variant(dev, h, p, v);
}
int yrtSetInt2(YRTDevice dev, YRTHandle h, const char* p, int x, int y) {
  Variant v; v.type = Variant::INT2; v.i[0] = x; v.i[1] = y;
  return set_variant(dev, h, p, v);
}
int yrtSetInt3(YRTDevice dev, YRTHandle h, const char* p, int x, int y, int z) {
  Variant v; v.type = Variant::INT3; v.i[0] = x; v.i[1] = y; v.i[2] = z;
  return set_variant(dev, h, p, v);
}
int yrtSetInt4(YRTDevice dev, YRTHandle h, const char* p, int x, int y, int z, int w) {
  Variant v; v.type = Variant::INT4; v.i[0] = x; v.i[1] = y; v.i[2] = z; v.i[3] = w;
  return set_variant(dev, h, p, v);
}
int yrtSetFloat1(YRTDevice dev, YRTHandle h, const char* p, float x) {
  Variant v; v.type = Variant::FLOAT1; v.f[0] = x;
  return set_variant(dev, h, p, v);
}
int yrtSetFloat2(YRTDevice dev, YRTHandle h, const char* p, float x, float y) {
  Variant v; v.type = Variant::FLOAT2; v.f[0] = x; v.f[1] = y;
  return set_variant(dev, h, p, v);
}
int yrtSetFloat3(YRTDevice dev, YRTHandle h, const char* p, float x, float y, float z) {
  Variant v; v.type = Variant::FLOAT3; v.f[0] = x; v.f[1] = y; v.f[2] = z;
  return set_variant(dev, h, p, v);
}
int yrtSetFloat4(YRTDevice dev, YRTHandle h, const char* p, float x, float y, float z, float w) {
  Variant v; v.type = Variant::FLOAT4; v.f[0] = x; v.f[1] = y; v.f[2] = z; v.f[3] = w;
  return set_variant(dev, h, p, v);
}
int yrtGetFloat3(YRTDevice dev, YRTHandle h, const char* p, float* x, float* y, float* z) {
  DEV_GUARD(dev, -1)
  const Variant* v = dev->d->ref(h)->obj->parms.find(p);
  if (!v || v->type != Variant::FLOAT3) throw std::runtime_error(std::string("no float3 property ") + p);
  *x = v->f[0]; *y = v->f[1]; *z = v->f[2];
  return 0;
  DEV_END(-1)
}
// rtGetFloat1 / rtGetString / rtGetTransform (singleray_device.cpp:548-555, 616-622, 651-657):
// the reference reads the handle's current value; unset properties read as 0 / "" / identity.
int yrtGetFloat1(YRTDevice dev, YRTHandle h, const char* p, float* x) {
  DEV_GUARD(dev, -1)
  if (!h) return 0;
  const Variant* v = dev->d->ref(h)->obj->parms.find(p);
  *x = 0.f;
  if (v) {
    if (v->type >= Variant::FLOAT1 && v->type <= Variant::FLOAT4) *x = v->f[0];
    else if (v->type >= Variant::BOOL1 && v->type <= Variant::INT4) *x = (float)v->i[0];
  }
  return 0;
  DEV_END(-1)
}
int yrtGetString(YRTDevice dev, YRTHandle h, const char* p, char* buf, size_t bufSize) {
  DEV_GUARD(dev, -1)
  if (!h) return 0;
  const Variant* v = dev->d->ref(h)->obj->parms.find(p);
  const std::string str = (v && v->type == Variant::STRING) ? v->str : std::string();
  if (buf && bufSize) {
    const size_t n = std::min(bufSize - 1, str.size());
    memcpy(buf, str.data(), n);
    buf[n] = 0;
  }
  return (int)str.size();
  DEV_END(-1)
}
int yrtGetTransform(YRTDevice dev, YRTHandle h, const char* p, float* transform12) {
  DEV_GUARD(dev, -1)
  if (!h) return 0;
  const Variant* v = dev->d->ref(h)->obj->parms.find(p);
  static const float I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  memcpy(transform12, (v && v->type == Variant::TRANSFORM) ? v->f : I, sizeof(I));
  return 0;
  DEV_END(-1)
}
int yrtSetArray(YRTDevice dev, YRTHandle h, const char* p, const char* type, YRTHandle data, size_t size,
                size_t stride, size_t ofs) {
  DEV_GUARD(dev, -1)
  auto d = dev->d->get<DataObj>(data, "data");
  if (!d) throw std::runtime_error("invalid data handle");
  Variant v;
  v.type = Variant::DATA;
  v.obj = d;
  v.dataType = type;
  v.size = size;
  size_t es = 0;
  if (ieq(type, "float2")) es = 8;
  else if (ieq(type, "float3") || ieq(type, "int3")) es = 12;
  else if (ieq(type, "float4") || ieq(type, "int4")) es = 16;
  else if (ieq(type, "float1") || ieq(type, "int1")) es = 4;
  else if (ieq(type, "int2")) es = 8;
  else throw std::runtime_error(std::string("unknown array type: ") + type);
  v.stride = stride == (size_t)-1 ? es : stride;
  v.ofs = ofs;
  if (size && v.ofs + (size - 1) * v.stride + es > d->bytes.size()) throw std::runtime_error("array exceeds data");
  dev->d->ref(h)->obj->parms.set(p, v);
  return 0;
  DEV_END(-1)
}
int yrtSetString(YRTDevice dev, YRTHandle h, const char* p, const char* str) {
  Variant v; v.type = Variant::STRING; v.str = str ? str : "";
  return set_variant(dev, h, p, v);
}
int yrtSetImage(YRTDevice dev, YRTHandle h, const char* p, YRTHandle image) {
  DEV_GUARD(dev, -1)
  Variant v;
  v.type = Variant::IMAGE;
  v.obj = dev->d->get<ImageObj>(image, "image");
  dev->d->ref(h)->obj->parms.set(p, v);
  return 0;
  DEV_END(-1)
}
int yrtSetTexture(YRTDevice dev, YRTHandle h, const char* p, YRTHandle texture) {
  DEV_GUARD(dev, -1)
  Variant v;
  v.type = Variant::TEXTURE;
  v.obj = dev->d->get<TextureObj>(texture, "texture");
  dev->d->ref(h)->obj->parms.set(p, v);
  return 0;
  DEV_END(-1)
}
int yrtSetTransform(YRTDevice dev, YRTHandle h, const char* p, const float* t) {
  Variant v;
  v.type = Variant::TRANSFORM;
  for (int i = 0; i < 12; ++i) v.f[i] = t[i];
  return set_variant(dev, h, p, v);
}
int yrtSetPointer(YRTDevice dev, YRTHandle h, const char* p, void* ptr) {
  Variant v; v.type = Variant::POINTER; v.ptr = ptr;
  return set_variant(dev, h, p, v);
}
int yrtClear(YRTDevice dev, YRTHandle h) {
  DEV_GUARD(dev, -1)
  dev->d->ref(h)->obj->parms.clear();
  return 0;
  DEV_END(-1)
}
int yrtCommit(YRTDevice dev, YRTHandle h) {
  DEV_GUARD(dev, -1)
  if (dev->d->gpu) HIP_CHECK(hipSetDevice(dev->d->hipDevice));
  dev->d->ref(h)->obj->commit();
  return 0;
  DEV_END(-1)
}

int yrtRenderFrame(YRTDevice dev, YRTHandle renderer, YRTHandle camera, YRTHandle scene, YRTHandle tonemapper,
                   YRTHandle framebuffer, int accumulate) {
  DEV_GUARD(dev, -1)
  std::shared_ptr<RendererObj> R;
  std::shared_ptr<CameraObj> C;
  std::shared_ptr<SceneObj> S;
  std::shared_ptr<ToneMapperObj> T;
  std::shared_ptr<FrameBufferObj> F;
  try {
    R = dev->d->get<RendererObj>(renderer, "renderer");
    C = dev->d->get<CameraObj>(camera, "camera");
    S = dev->d->get<SceneObj>(scene, "scene");
    T = dev->d->get<ToneMapperObj>(tonemapper, "tonemapper");
    F = dev->d->get<FrameBufferObj>(framebuffer, "framebuffer");
    if (!R || !C || !S || !T || !F) throw std::runtime_error("rtRenderFrame: null handle");
    if (!dev->d->gpu) throw std::runtime_error("rtRenderFrame: host-only device (created with parms \"host\")");
  } catch (...) {
    dev->d->fail_proc_gather();  // the peers of a process gather must not wait for this rank
    throw;
  }
  dev->d->render(*R, {C.get()}, *S, *T, {F.get()}, accumulate);
  return 0;
  DEV_END(-1)
}

int yrtRenderFrames(YRTDevice dev, YRTHandle renderer, const YRTHandle* cameras, int numFrames, YRTHandle scene,
                    YRTHandle tonemapper, const YRTHandle* framebuffers, int accumulate) {
  DEV_GUARD(dev, -1)
  std::shared_ptr<RendererObj> R;
  std::shared_ptr<SceneObj> S;
  std::shared_ptr<ToneMapperObj> T;
  std::vector<std::shared_ptr<CameraObj>> cs;
  std::vector<std::shared_ptr<FrameBufferObj>> fs;
  std::vector<CameraObj*> cp;
  std::vector<FrameBufferObj*> fp;
  try {
    if (numFrames < 1 || !cameras || !framebuffers) throw std::runtime_error("rtRenderFrames: no frames");
    R = dev->d->get<RendererObj>(renderer, "renderer");
    S = dev->d->get<SceneObj>(scene, "scene");
    T = dev->d->get<ToneMapperObj>(tonemapper, "tonemapper");
    if (!R || !S || !T) throw std::runtime_error("rtRenderFrames: null handle");
    // one accumulation state per framebuffer and sampler iteration per job: a multi-frame job
    // equals a loop of yrtRenderFrame calls only for non-accumulating frames (yrt_device.h)
    if (numFrames > 1 && accumulate) throw std::runtime_error("rtRenderFrames: accumulate needs numFrames == 1");
    cs.resize(numFrames);
    fs.resize(numFrames);
    cp.resize(numFrames);
    fp.resize(numFrames);
    for (int k = 0; k < numFrames; ++k) {
      cs[k] = dev->d->get<CameraObj>(cameras[k], "camera");
      fs[k] = dev->d->get<FrameBufferObj>(framebuffers[k], "framebuffer");
      if (!cs[k] || !fs[k]) throw std::runtime_error("rtRenderFrames: null camera or framebuffer handle");
      cp[k] = cs[k].get();
      fp[k] = fs[k].get();
    }
    if (!dev->d->gpu) throw std::runtime_error("rtRenderFrames: host-only device (created with parms \"host\")");
  } catch (...) {
    dev->d->fail_proc_gather();
    throw;
  }
  dev->d->render(*R, cp, *S, *T, fp, accumulate);
  return 0;
  DEV_END(-1)
}

void* yrtMapFrameBuffer(YRTDevice dev, YRTHandle fb, int bufID) {
  DEV_GUARD(dev, nullptr)
  auto F = dev->d->get<FrameBufferObj>(fb, "framebuffer");
  const int id = bufID < 0 ? F->cur : bufID;
  if (id < 0 || id >= F->depth) throw std::runtime_error("rtMapFrameBuffer: invalid buffer id");
  fb_read_back(*F, id);  // a frame still in HBM comes to the host pixels now
  return F->buffer(id);
  DEV_END(nullptr)
}
int yrtUnmapFrameBuffer(YRTDevice dev, YRTHandle fb, int) {
  DEV_GUARD(dev, -1)
  (void)dev->d->get<FrameBufferObj>(fb, "framebuffer");
  return 0;
  DEV_END(-1)
}
int yrtSwapBuffers(YRTDevice dev, YRTHandle fb) {
  DEV_GUARD(dev, -1)
  auto F = dev->d->get<FrameBufferObj>(fb, "framebuffer");
  F->cur = (F->cur + 1) % F->depth;
  return 0;
  DEV_END(-1)
}
int yrtSetStatusCallback(YRTDevice dev, YRTHandle renderer, YRTStatusCallback cb, void* user) {
  DEV_GUARD(dev, -1)
  auto R = dev->d->get<RendererObj>(renderer, "renderer");
  R->statusCallback = (void*)cb;
  R->statusUser = user;
  return 0;
  DEV_END(-1)
}
int yrtSetStopFlag(YRTDevice dev, YRTHandle renderer, volatile int* flag) {
  DEV_GUARD(dev, -1)
  auto R = dev->d->get<RendererObj>(renderer, "renderer");
  R->stopFlag = (std::atomic<bool>*)flag;  // polled as a byte-sized bool between batches
  return 0;
  DEV_END(-1)
}

int yrtIntersectTimed(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, const float* time,
                      uint32_t n, float* hit4, void* stream) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  dev->d->intersect(*S, org4, dir4, time, n, hit4, nullptr, stream ? (hipStream_t)stream : dev->d->stream);
  return 0;
  DEV_END(-1)
}
int yrtOccludedTimed(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, const float* time,
                     uint32_t n, int32_t* occ, void* stream) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  dev->d->intersect(*S, org4, dir4, time, n, nullptr, occ, stream ? (hipStream_t)stream : dev->d->stream);
  return 0;
  DEV_END(-1)
}
int yrtIntersect(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, uint32_t n, float* hit4,
                 void* stream) {
  return yrtIntersectTimed(dev, scene, org4, dir4, nullptr, n, hit4, stream);
}
int yrtOccluded(YRTDevice dev, YRTHandle scene, const float* org4, const float* dir4, uint32_t n, int32_t* occ,
                void* stream) {
  return yrtOccludedTimed(dev, scene, org4, dir4, nullptr, n, occ, stream);
}
int yrtTriangleIds(YRTDevice dev, YRTHandle scene, int32_t tri, int32_t* geomID, int32_t* primID) {
  DEV_GUARD(dev, -1)
  auto S = dev->d->get<SceneObj>(scene, "scene");
  if (!S->gpu) throw std::runtime_error("scene not committed");
  if (tri < 0 || tri >= S->gpu->numTris) { *geomID = -1; *primID = -1; return 0; }
  const int g = S->gpu->hTriGeom[tri];
  *geomID = g;
  *primID = tri - S->gpu->hGeoms[g].triBase;
  return 0;
  DEV_END(-1)
}
int yrtPick(YRTDevice dev, YRTHandle camera, float x, float y, YRTHandle scene, float* px, float* py, float* pz) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("rtPick: host-only device");
  auto C = D.get<CameraObj>(camera, "camera");
  auto S = D.get<SceneObj>(scene, "scene");
  if (!C || !S || !S->gpu) throw std::runtime_error("rtPick: invalid camera or uncommitted scene");
  HIP_CHECK(hipSetDevice(D.hipDevice));
  GpuCtx& g = *D.ctx[0];
  g.dCam.alloc(sizeof(GpuCamera));
  g.dCount.alloc(sizeof(float4));
  HIP_CHECK(hipMemcpyAsync(g.dCam.p, &C->cam, sizeof(GpuCamera), hipMemcpyHostToDevice, D.stream));
  launch_pick(S->gpu->view, g.dCam.as<GpuCamera>(), x, y, g.dCount.as<float4>(), D.stream);
  float4 r;
  HIP_CHECK(hipMemcpyAsync(&r, g.dCount.p, sizeof(r), hipMemcpyDeviceToHost, D.stream));
  HIP_CHECK(hipStreamSynchronize(D.stream));
  *px = r.x;
  *py = r.y;
  *pz = r.z;
  return __builtin_bit_cast(int, r.w) >= 0 ? 1 : 0;
  DEV_END(-1)
}

// The library's YRTDenoiseParams: the defaults overlaid by the fields the caller's struct holds.
// sigmaColor 1: the lowest mean squared error against a 1024-spp frame, summed over C1 and C2,
// among 0.25, 0.5, 1, 2 and off. albedoFloor 1/255: the 8-bit texel quantum, the
// smallest non-zero albedo an 8-bit texture can hold (§9).
static YRTDenoiseParams denoise_params(const YRTDenoiseParams* p) {
  YRTDenoiseParams d;
  d.size = (uint32_t)sizeof(YRTDenoiseParams);
  d.iterations = 5;
  d.sigmaColor = 1.0f;
  d.sigmaNormal = 64.f;
  d.sigmaPosition = 0.02f;
  d.demodulate = 0;
  d.albedoPower = 1.0f;
  d.albedoFloor = 1.0f / 255.0f;
  // sigmaVariance 3: the lowest sum of the four below-1 error ratios (C1 and C2 after 2 and 8
  // iterations) among 1, 2, 3, 4 in the CPU rehearsal (tools/denoise_variance_rehearsal.py, §9).
  // varianceFloor (1/255)^2: the square of an 8-bit step, so a byte frame's quantisation never
  // reads as signal.
  d.varianceGuided = 0;
  d.sigmaVariance = 3.0f;
  d.varianceFloor = (1.0f / 255.0f) * (1.0f / 255.0f);
  if (!p) return d;
  if (p->size < sizeof(uint32_t)) throw std::runtime_error("YRTDenoiseParams: size is smaller than the size field");
  const size_t n = p->size;
#define YRT_DN_FIELD(f) \
  if (n >= offsetof(YRTDenoiseParams, f) + sizeof(d.f)) d.f = p->f
  YRT_DN_FIELD(iterations);
  YRT_DN_FIELD(sigmaColor);
  YRT_DN_FIELD(sigmaNormal);
  YRT_DN_FIELD(sigmaPosition);
  YRT_DN_FIELD(demodulate);
  YRT_DN_FIELD(albedoPower);
  YRT_DN_FIELD(albedoFloor);
  YRT_DN_FIELD(varianceGuided);
  YRT_DN_FIELD(sigmaVariance);
  YRT_DN_FIELD(varianceFloor);
#undef YRT_DN_FIELD
  if (d.iterations < 0 || d.iterations > 16) throw std::runtime_error("YRTDenoiseParams: iterations outside 0..16");
  if (!(d.sigmaNormal >= 0.f) || !(d.sigmaPosition > 0.f) || d.sigmaColor != d.sigmaColor)
    throw std::runtime_error("YRTDenoiseParams: sigmaNormal >= 0 and sigmaPosition > 0 are required");
  const auto positive = [](float v) { return v > 0.f && v <= 3.40282347e38f; };
  if (d.demodulate != 0 && !positive(d.albedoPower))
    throw std::runtime_error("YRTDenoiseParams: demodulate needs a finite albedoPower > 0");
  if (d.demodulate != 0 && !positive(d.albedoFloor))
    throw std::runtime_error("YRTDenoiseParams: demodulate needs a finite albedoFloor > 0");
  if (d.varianceGuided != 0 && !positive(d.sigmaVariance))
    throw std::runtime_error("YRTDenoiseParams: varianceGuided needs a finite sigmaVariance > 0");
  if (d.varianceGuided != 0 && !positive(d.varianceFloor))
    throw std::runtime_error("YRTDenoiseParams: varianceGuided needs a finite varianceFloor > 0");
  return d;
}

int yrtDenoiseDefaults(YRTDenoiseParams* p) {
  if (!p || p->size < sizeof(uint32_t)) return -1;
  const YRTDenoiseParams d = denoise_params(nullptr);
  memcpy((char*)p + sizeof(uint32_t), (const char*)&d + sizeof(uint32_t),
         std::min<size_t>(p->size, sizeof(d)) - sizeof(uint32_t));
  return 0;
}

// yrtRenderGuides / yrtRenderAlbedo: the guide pass of one width x height view, then each frame
// of `out` (a guide buffer of ctx[0], the host frame it goes to) copied to the host
static void render_guides(Device& D, const char* what, YRTHandle camera, YRTHandle scene, int width, int height,
                          bool albedo, std::initializer_list<std::pair<DevBuf GpuCtx::*, float*>> out) {
  if (!D.gpu) throw std::runtime_error(std::string(what) + ": host-only device (created with parms \"host\")");
  auto C = D.get<CameraObj>(camera, "camera");
  auto S = D.get<SceneObj>(scene, "scene");
  bool null = !C || !S;
  for (const auto& o : out) null = null || !o.second;
  if (null) throw std::runtime_error(std::string(what) + ": null handle or pointer");
  if (width < 1 || height < 1) throw std::runtime_error(std::string(what) + ": empty frame");
  D.guides({C.get()}, *S, width, height, what, albedo);
  const size_t bytes = (size_t)width * height * sizeof(float4);
  for (const auto& o : out)
    HIP_CHECK(hipMemcpyAsync(o.second, ((*D.ctx[0]).*o.first).p, bytes, hipMemcpyDeviceToHost, D.stream));
  HIP_CHECK(hipStreamSynchronize(D.stream));
  D.evGuides.read(D.msGuides);
}

int yrtRenderGuides(YRTDevice dev, YRTHandle camera, YRTHandle scene, int width, int height, float* pos4Host,
                    float* nrm4Host) {
  DEV_GUARD(dev, -1)
  render_guides(*dev->d, "yrtRenderGuides", camera, scene, width, height, false,
                {{&GpuCtx::dGuidePos, pos4Host}, {&GpuCtx::dGuideNrm, nrm4Host}});
  return 0;
  DEV_END(-1)
}

int yrtRenderAlbedo(YRTDevice dev, YRTHandle camera, YRTHandle scene, int width, int height, float* albedo4Host) {
  DEV_GUARD(dev, -1)
  render_guides(*dev->d, "yrtRenderAlbedo", camera, scene, width, height, true, {{&GpuCtx::dGuideAlbedo, albedo4Host}});
  return 0;
  DEV_END(-1)
}

int yrtDenoiseFrameBuffer(YRTDevice dev, YRTHandle camera, YRTHandle scene, YRTHandle framebuffer,
                          const YRTDenoiseParams* p) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  const YRTDenoiseParams dp = denoise_params(p);
  if (!D.gpu) throw std::runtime_error("yrtDenoiseFrameBuffer: host-only device (created with parms \"host\")");
  auto C = D.get<CameraObj>(camera, "camera");
  auto S = D.get<SceneObj>(scene, "scene");
  auto F = D.get<FrameBufferObj>(framebuffer, "framebuffer");
  if (!C || !S || !F) throw std::runtime_error("yrtDenoiseFrameBuffer: null handle");
  D.denoise({C.get()}, *S, {F.get()}, dp, false, "yrtDenoiseFrameBuffer");
  return 0;
  DEV_END(-1)
}

// Validation first (it needs no GPU), then the host-only refusal, then the filter. The slots are
// ordered eye-major, face-minor: slot = eye * 6 + cubeFaceIndex % 6 (one eye: slots 0..5).
int yrtDenoiseCube(YRTDevice dev, const YRTHandle* cameras, int numFrames, YRTHandle scene,
                   const YRTHandle* framebuffers, const YRTDenoiseParams* p) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  const YRTDenoiseParams dp = denoise_params(p);
  if (numFrames != 6 && numFrames != 12)
    throw std::runtime_error("yrtDenoiseCube: numFrames must be 6 (one eye) or 12, got " + std::to_string(numFrames));
  if (!cameras || !framebuffers) throw std::runtime_error("yrtDenoiseCube: null camera or framebuffer array");
  auto S = D.get<SceneObj>(scene, "scene");
  if (!S) throw std::runtime_error("yrtDenoiseCube: null handle");
  std::vector<std::shared_ptr<CameraObj>> camRefs(numFrames);
  std::vector<std::shared_ptr<FrameBufferObj>> fbRefs(numFrames);
  std::vector<CameraObj*> C(numFrames, nullptr);
  std::vector<FrameBufferObj*> F(numFrames, nullptr);
  int firstEye = -1;
  for (int k = 0; k < numFrames; ++k) {
    camRefs[k] = D.get<CameraObj>(cameras[k], "camera");
    fbRefs[k] = D.get<FrameBufferObj>(framebuffers[k], "framebuffer");
    if (!camRefs[k] || !fbRefs[k]) throw std::runtime_error("yrtDenoiseCube: null handle");
    const GpuCamera& cam = camRefs[k]->cam;
    if (!ieq(camRefs[k]->type.c_str(), "stereo") || cam.type != CAM_STEREO)
      throw std::runtime_error("yrtDenoiseCube: camera " + std::to_string(k) + " is not a committed \"stereo\" camera");
    if (cam.cubeFaceIndex < 0 || cam.cubeFaceIndex > 11)
      throw std::runtime_error("yrtDenoiseCube: camera " + std::to_string(k) + " has a cubeFaceIndex outside 0..11");
    const int eye = cam.cubeFaceIndex / 6, face = cam.cubeFaceIndex % 6;
    if (firstEye < 0) firstEye = eye;
    if (numFrames == 6 && eye != firstEye)
      throw std::runtime_error("yrtDenoiseCube: 6 frames must be the six faces of one eye; camera " + std::to_string(k) +
                               " belongs to the other eye, so a face is missing");
    const int slot = (numFrames == 6 ? 0 : eye * 6) + face;
    if (C[slot])
      throw std::runtime_error("yrtDenoiseCube: face " + std::to_string(face) + " of the " + (eye ? "right" : "left") +
                               " eye appears twice, so another face is missing");
    C[slot] = camRefs[k].get();
    F[slot] = fbRefs[k].get();
  }
  for (int e = 0; e < numFrames / 6; ++e) {
    GpuCamera first = C[6 * e]->cam;
    first.cubeFaceIndex = 0;
    for (int f = 1; f < 6; ++f) {
      GpuCamera other = C[6 * e + f]->cam;
      other.cubeFaceIndex = 0;
      if (memcmp(&first, &other, sizeof(GpuCamera)) != 0)
        throw std::runtime_error("yrtDenoiseCube: the cameras of one eye differ in more than cubeFaceIndex (face " +
                                 std::to_string(f) + " against face 0)");
    }
    const std::string defect = cube_cameras_defect(C[6 * e]->cam);
    if (!defect.empty()) throw std::runtime_error("yrtDenoiseCube: " + defect);
  }
  const int W = F[0]->width;
  for (int k = 0; k < numFrames; ++k) {
    if (F[k]->width != F[k]->height || F[k]->width < 1)
      throw std::runtime_error("yrtDenoiseCube: a cube face's framebuffer must be square");
    if (F[k]->width != W || F[k]->format != F[0]->format)
      throw std::runtime_error("yrtDenoiseCube: the framebuffers must have one size and one format");
    for (int j = 0; j < k; ++j)
      if (F[j] == F[k]) throw std::runtime_error("yrtDenoiseCube: a framebuffer appears twice");
  }
  if (W > YRT_CUBE_MAX_WIDTH) throw std::runtime_error("yrtDenoiseCube: faces wider than 16384 pixels");
  if (!D.gpu) throw std::runtime_error("yrtDenoiseCube: host-only device (created with parms \"host\")");
  D.denoise(C, *S, F, dp, true, "yrtDenoiseCube");
  return 0;
  DEV_END(-1)
}

int yrtFrameVariance(YRTDevice dev, YRTHandle framebuffer, float* var4Host) {
  DEV_GUARD(dev, -1)
  Device& D = *dev->d;
  if (!D.gpu) throw std::runtime_error("yrtFrameVariance: host-only device (created with parms \"host\")");
  auto F = D.get<FrameBufferObj>(framebuffer, "framebuffer");
  if (!F || !var4Host) throw std::runtime_error("yrtFrameVariance: null handle or pointer");
  D.frame_variance(*F, var4Host);
  return 0;
  DEV_END(-1)
}

int yrtGetFrameBufferSize(YRTDevice dev, YRTHandle framebuffer, int* width, int* height) {
  DEV_GUARD(dev, -1)
  auto F = dev->d->get<FrameBufferObj>(framebuffer, "framebuffer");
  if (!F) throw std::runtime_error("yrtGetFrameBufferSize: null handle");
  if (width) *width = F->width;
  if (height) *height = F->height;
  return 0;
  DEV_END(-1)
}

int yrtDebugFrameVariance(const float* accu4, const float* half4, int width, int height, float gamma, int vignetting,
                          float* var4) {
  if (!accu4 || !half4 || !var4 || width < 1 || height < 1) return -1;
  const float rcpGamma = rcpf_(gamma);  // as the render's resolve has it
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const size_t o = ((size_t)y * width + x) * 4;
      yrt_pixel_variance(accu4 + o, half4 + o, x, y, width, height, gamma, rcpGamma, vignetting ? 1 : 0, var4 + o);
    }
  return 0;
}

int yrtGetDenoiseTimes(YRTDevice dev, float* msGuides, float* msFilter) {
  DEV_GUARD(dev, -1)
  if (msGuides) *msGuides = dev->d->msGuides;
  if (msFilter) *msFilter = dev->d->msFilter;
  return 0;
  DEV_END(-1)
}

}  // extern "C"
