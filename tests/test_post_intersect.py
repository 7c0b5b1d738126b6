"""postIntersect's two vertex sources on the same triangles (csrc/kernels/yrt_surface.h): a static
mesh reads its GpuTriShade record, a mesh with a `motions` array (GF_MOTION) the index record and
the vertex arrays. A `motions` array of zeros moves nothing, so the one scene built with and
without it must give the same frame, guides, albedo and ray counts, bit for bit, and each variant
its oracle image.

The scene: one trianglemesh of four triangles (a bent, tilted strip of two quads, no two vertices
sharing a coordinate, a different normal at every vertex, texture coordinates) used by two
primitives, one MatteTextured over an 8 x 8 image and one BrushedMetal (the derived tangents,
wantTangents without tangent arrays), under an ambient and a triangle light."""
import numpy as np
import pytest

import oracle
from helpers import parity

W = 64
F = np.float32


def _scene(d, zero_motion):
    from test_cpu_host import yrt_lookat
    import denoise_albedo_ref as aref
    pos = np.array([[-151, 12, -290], [4, -35, -305], [148, 22, -281],
                    [-143, 41, 301], [-9, 68, 285], [156, 5, 310]], F)
    nor = np.array([[0.10, 1, 0.05], [-0.22, 1, 0.12], [0.31, 1, -0.17],
                    [-0.08, 1, -0.26], [0.19, 1, 0.23], [-0.35, 1, 0.04]], F)
    nor /= np.linalg.norm(nor, axis=1, keepdims=True).astype(F)
    uv = np.array([[0.03, 0.06], [0.48, 0.02], [0.97, 0.09], [0.05, 0.93], [0.53, 0.98], [0.94, 0.91]], F)
    idx = np.array([[0, 4, 1], [0, 3, 4], [1, 5, 2], [1, 4, 5]], np.int32)
    arrays = [("positions", pos, "float3"), ("normals", nor, "float3"), ("texcoords", uv, "float2"),
              ("indices", idx, "int3")]
    if zero_motion:
        arrays.append(("motions", np.zeros((6, 3), F), "float3"))
    mesh = d.rtNewShape("trianglemesh")
    for name, arr, typ in arrays:
        d.rtSetArray(mesh, name, typ, d.rtNewData("immutable", arr), len(arr), arr.itemsize * arr.shape[1])
    d.rtCommit(mesh)
    matte = aref.material(d, "MatteTextured", textures=[("Kd", aref.texture(d, "bilinear", aref.texture_image(8)))])
    metal = aref.material(d, "BrushedMetal", [("reflectance", (0.9, 0.8, 0.6)), ("roughnessX", 0.02),
                                              ("roughnessY", 0.5)])
    amb = d.rtNewLight("ambientlight")
    d.rtSetFloat3(amb, "L", 0.3, 0.3, 0.35)
    d.rtCommit(amb)
    tl = d.rtNewLight("trianglelight")
    for n, v in (("v0", (-60, 200, -60)), ("v1", (60, 200, -60)), ("v2", (0, 200, 80)), ("L", (40, 38, 30))):
        d.rtSetFloat3(tl, n, *v)
    d.rtCommit(tl)
    scene = d.rtNewScene("default")
    move = lambda x, y, z: (1, 0, 0, 0, 1, 0, 0, 0, 1, x, y, z)
    d.rtSetPrimitive(scene, 0, d.rtNewShapePrimitive(mesh, matte, move(-158, 3, 7)))
    d.rtSetPrimitive(scene, 1, d.rtNewShapePrimitive(mesh, metal, move(161, -4, -6)))
    d.rtSetPrimitive(scene, 2, d.rtNewLightPrimitive(amb))
    d.rtSetPrimitive(scene, 3, d.rtNewLightPrimitive(tl))
    d.rtCommit(scene)
    cam = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam, "local2world", yrt_lookat((0, 250, -420), (0, 0, 0), (0, 1, 0)))
    d.rtSetFloat1(cam, "angle", 60.0)
    d.rtSetFloat1(cam, "aspectRatio", 1.0)
    d.rtCommit(cam)
    r = d.rtNewRenderer("pathtracer")
    d.rtSetInt1(r, "maxDepth", 3)
    d.rtSetInt1(r, "sampler.spp", 8)
    d.rtSetFloat1(r, "tMaxShadowRay", 1e4)
    d.rtCommit(r)
    tm = d.rtNewToneMapper("default")
    d.rtCommit(tm)
    return r, cam, scene, tm


def test_zero_motion_leaves_the_oracle_image(host_device):
    """The premise: in the reference arithmetic p + t * 0 is p, so the oracle renders the two
    variants' frame blobs to the same image (and the blobs do differ: one carries motions)."""
    d = host_device
    imgs = []
    for zero_motion in (False, True):
        r, cam, scene, _ = _scene(d, zero_motion)
        blob = d.export_frame(r, cam, scene)
        assert (b"motions" in blob) == zero_motion
        imgs.append(oracle.render(blob, W, W, 1.0)[0])
    assert np.isfinite(imgs[0]).all() and imgs[0].std() > 0
    assert np.array_equal(imgs[0], imgs[1])


@pytest.fixture(scope="module")
def variants(gpu_device):
    """Per variant (static, zero motion): frame, oracle image, ray counts, pos4, nrm4, albedo4."""
    d = gpu_device
    out = []
    for zero_motion in (False, True):
        r, cam, scene, tm = _scene(d, zero_motion)
        fb = d.rtNewFrameBuffer("RGB_FLOAT32", W, W)
        d.rtRenderFrame(r, cam, scene, tm, fb, 0)
        st = d.render_stats()
        v = {"frame": d.framebuffer_array(fb, W, W, "RGB_FLOAT32").copy(),
             "rays": (st["raysClosest"], st["raysShadow"]),
             "ref": oracle.render(d.export_frame(r, cam, scene), W, W, 1.0)[0]}
        v["pos"], v["nrm"] = d.render_guides(cam, scene, W, W)
        v["albedo"] = d.render_albedo(cam, scene, W, W)
        out.append(v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["static", "zero_motion"])
def test_each_source_matches_the_oracle(variants, variant):
    v = variants[variant]
    parity(v["frame"], v["ref"], 0.999, exact=True)


@pytest.mark.gpu
def test_the_two_sources_give_the_same_frame(variants):
    a, b = variants
    assert np.array_equal(a["frame"], b["frame"])
    assert a["rays"] == b["rays"] and a["rays"][0] > 0 and a["rays"][1] > 0


@pytest.mark.gpu
def test_the_two_sources_give_the_same_guides(variants):
    """k_guides reads the record of the static mesh and the vertex arrays of the other; both
    primitives are in view, so the texture lookup at (s, t) and the interpolated Ns are compared."""
    a, b = variants
    hit = np.isfinite(a["pos"][..., 3])
    assert 0.2 < hit.mean() < 1.0
    assert len(np.unique(a["albedo"][hit][:, :3], axis=0)) > 16  # the texture shows
    for k in ("pos", "nrm", "albedo"):
        assert np.array_equal(a[k], b[k]), k
