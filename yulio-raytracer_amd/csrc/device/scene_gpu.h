// scene_gpu.h — a committed scene flattened into HBM (layout: common/yrt_gpu_types.h): its device
// buffers (SceneBuffers, listed once), host mirrors and refit tables; build, peer copy, refit.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <iterator>
#include <memory>
#include <vector>

#include "../kernels/yrt_kernels.h"
#include "bvh_build.h"
#include "dev_buf.h"
#include "objects.h"
#include "sampler.h"

namespace yrt {

// The device buffers of a scene that its replica on another GPU needs too: what SceneView points
// at, and the float nodes. `all` is the one list of them: replicate_gpu_scene copies what it names,
// in that order, and bind_view (scene_gpu.cpp) gives the buffers their types. A buffer declared
// here without an entry in `all` fails the static_assert below.
struct SceneBuffers {
  DevBuf nodes, qnodes, tris, triGeom, indices, positions, normals, texcoords, geoms, materials, textures, images, texels, texQuads,
      lights, envLights, media, geomRecs, motions, tangents, triMotion, triShade;
  static constexpr DevBuf SceneBuffers::*all[] = {
      &SceneBuffers::nodes,     &SceneBuffers::qnodes,    &SceneBuffers::tris,     &SceneBuffers::triGeom,
      &SceneBuffers::indices,   &SceneBuffers::positions, &SceneBuffers::normals,  &SceneBuffers::texcoords,
      &SceneBuffers::geoms,     &SceneBuffers::geomRecs,  &SceneBuffers::triShade, &SceneBuffers::materials,
      &SceneBuffers::textures,  &SceneBuffers::images,    &SceneBuffers::texels,   &SceneBuffers::texQuads,
      &SceneBuffers::lights,    &SceneBuffers::envLights, &SceneBuffers::media,    &SceneBuffers::motions,
      &SceneBuffers::triMotion, &SceneBuffers::tangents};
};
static_assert(sizeof(SceneBuffers) == std::size(SceneBuffers::all) * sizeof(DevBuf),
              "every DevBuf of SceneBuffers needs an entry in SceneBuffers::all (a replica would miss it)");

struct GpuScene : SceneBuffers {
  int device = 0;
  uint64_t serial = next_serial();  // identifies the committed scene in caches (addresses get reused)
  static uint64_t next_serial() {
    static std::atomic<uint64_t> n{1};
    return n++;
  }
  bool hasMotion = false;  // moving geometry: time-aware trace kernels, no refit
  SceneView view{};
  unsigned materialMask = 0;  // bit MAT_x per material type, bit 16+LIGHT_x per light type used (shade kernel variant)
  size_t texels8Bytes = 0;    // the 8-bit images' part of the texel pool (float images follow it)
  size_t texelsBytes = 0;     // the whole pool
  // host mirrors of the small shading tables (the debug probes' bounds checks and pool export);
  // hTexels: the texel pool of a host-only scene, which has no device copy
  std::vector<GpuMaterial> hMaterials;
  std::vector<GpuTexture> hTextures;
  std::vector<GpuImage> hImages;
  std::vector<float4> hMedia;
  std::vector<uint8_t> hTexels;
  // host mirrors (BVH export, precomputed light sampling, stats)
  std::vector<GpuNode> hNodes;
  std::vector<GpuQNode> hQNodes;  // the same tree with 64-B quantized nodes (common/yrt_qnode.h)
  std::vector<GpuTri> hTris;
  std::vector<GpuGeom> hGeoms;
  std::vector<int> hTriGeom;
  std::vector<std::shared_ptr<const LightInst>> allLights;
  std::vector<GpuLight> hLights;                // the uploaded light table
  std::vector<int> hEnvLights;                  // the uploaded envLights (indices into hLights)
  std::vector<LightSampleSource> precomputed;   // LightSampleSource per precompute() light
  // incremental commits (faceCamera refit, refit_gpu_scene): the slots this scene was built
  // from, slot -> geometry, gid -> leaf position, and the node indices grouped by tree depth
  std::vector<std::shared_ptr<ScenePrim>> slotsCommitted;
  std::vector<int> slotGeom;
  std::vector<int> levelStart;  // nodes of depth d: levelNodes[levelStart[d] .. levelStart[d+1])
  // the refit kernels' tables: with the primary only, outside SceneBuffers::all on purpose (a
  // refit runs on the primary, whose replicas are then copied again)
  DevBuf triLeaf, levelNodes;
  bool hostBvhStale = false;    // hNodes/hTris lag a device refit until sync_host_bvh
  int refits = 0;               // refit commits since the build (stats)
  int numTris = 0, numGeoms = 0, bvhDepth = 0;
  double buildSeconds = 0;
  bool mortonAsked = false;     // the builder this tree was asked of (a commit that asks for the other one rebuilds)
  BuildInfo buildInfo;          // the BVH step of the build (yrtGetSceneBuildInfo)
  float bboxLo[3] = {0, 0, 0}, bboxHi[3] = {0, 0, 0};
};

// The device record of a world-space light without the scene's own indices (image, precomputed
// slot): what the light samplers read. build_gpu_scene fills those in.
GpuLight gpu_light_record(const LightInst& L);

// The 2x2 footprint records of the pool's 8-bit images (texQuads): one 16-byte record per texel,
// 4 x texels8Bytes in all, as uint32 words.
std::vector<uint32_t> build_tex_quads(const std::vector<GpuImage>& images, const std::vector<uint8_t>& texels,
                                      size_t texels8Bytes);

// morton: the scene builder "morton" (bvh_build.h) instead of the host SAH builder: on the GPU in
// `stream` when the scene is uploaded, else its host loop; timing: HIP-event time of its kernels
std::shared_ptr<GpuScene> build_gpu_scene(const std::vector<std::shared_ptr<ScenePrim>>& prims, int stackDepth,
                                          bool upload, bool morton = false, hipStream_t stream = nullptr,
                                          bool timing = false);
// A copy of an uploaded scene's device buffers on another HIP device (peer copies over xGMI),
// for multi-GPU tile rendering; the host-side mirrors stay with the source.
std::shared_ptr<GpuScene> replicate_gpu_scene(const GpuScene& src, int device);
// Commits `prims` onto an uploaded scene without a rebuild when only vertex positions/normals
// of some primitives changed (faceCamera re-orientation): uploads the moved vertices and
// refits the BVH on the GPU. Returns false (scene untouched) when a rebuild is needed.
bool refit_gpu_scene(GpuScene& S, const std::vector<std::shared_ptr<ScenePrim>>& prims, hipStream_t stream);
// Brings the host BVH mirrors (export, stats) up to date after device refits.
void sync_host_bvh(GpuScene& S);

}  // namespace yrt
