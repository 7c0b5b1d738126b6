"""k_shade's grouped loads (csrc/kernels/k_shade.h, yrt_surface.h: TriRecordSource, geom_burst,
wave_append2): a hit's whole 96-byte shading record is loaded before its geometry is known, the
geometry record's fields in one group, and the queue reservations go out before any store. The
same values reach the same arithmetic, so every frame below equals the oracle's bit for bit.

1. every geometry kind through the record burst, the record at the end of the array included;
2. Uber's three specular branches (and a geometry without a material) from registers;
3. two direct lights (the unfused resolve: shFirst, sOcc, k_shadow_resolve) under one lane and
   under batch capacities that split the frame differently."""
import re

import numpy as np
import pytest

import oracle
import yrt
from helpers import SCENES, c2_args, parity

F = np.float32
QUAD_IDX = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
QUAD_UV = np.array([[0.04, 0.07], [0.95, 0.03], [0.97, 0.92], [0.06, 0.96]], F)
EYE, TARGET = (0.0, 250.0, -420.0), (0.0, 0.0, 0.0)


def _mesh(d, pos, idx=QUAD_IDX, normals=None, uv=None, motions=None):
    arrays = [("positions", np.asarray(pos, F), "float3"), ("indices", np.asarray(idx, np.int32), "int3")]
    if normals is not None:
        arrays.append(("normals", np.asarray(normals, F), "float3"))
    if uv is not None:
        arrays.append(("texcoords", np.asarray(uv, F), "float2"))
    if motions is not None:
        arrays.append(("motions", np.asarray(motions, F), "float3"))
    mesh = d.rtNewShape("trianglemesh")
    for name, arr, typ in arrays:
        d.rtSetArray(mesh, name, typ, d.rtNewData("immutable", arr), len(arr), arr.itemsize * arr.shape[1])
    d.rtCommit(mesh)
    return mesh


def _bent_quad(k):
    """A quad of two triangles about the origin, no two corners at one height, different per k."""
    return np.array([[-70, 3 * k, -70], [70, 10 + k, -70], [70, -5 - 2 * k, 70], [-70, 15 - k, 70]], F)


def _normals(k):
    n = np.array([[0.10, 1, 0.05 * k], [-0.22, 1, 0.12], [0.31, 1, -0.17], [-0.08 * k, 1, -0.26]], F)
    return n / np.linalg.norm(n, axis=1, keepdims=True).astype(F)


def _move(x, y, z, s=1.0):
    return (s, 0, 0, 0, s, 0, 0, 0, s, x, y, z)


def _lights(d, scene, slot):
    amb = d.rtNewLight("ambientlight")
    d.rtSetFloat3(amb, "L", 0.3, 0.3, 0.35)
    d.rtCommit(amb)
    tl = d.rtNewLight("trianglelight")
    for n, v in (("v0", (-60, 300, -60)), ("v1", (60, 300, -60)), ("v2", (0, 300, 80)), ("L", (60, 57, 45))):
        d.rtSetFloat3(tl, n, *v)
    d.rtCommit(tl)
    d.rtSetPrimitive(scene, slot, d.rtNewLightPrimitive(amb))
    d.rtSetPrimitive(scene, slot + 1, d.rtNewLightPrimitive(tl))


def _finish(d, scene, depth, spp):
    from test_cpu_host import yrt_lookat
    d.rtCommit(scene)
    cam = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam, "local2world", yrt_lookat(EYE, TARGET, (0, 1, 0)))
    d.rtSetFloat1(cam, "angle", 60.0)
    d.rtSetFloat1(cam, "aspectRatio", 1.0)
    d.rtCommit(cam)
    r = d.rtNewRenderer("pathtracer")
    d.rtSetInt1(r, "maxDepth", depth)
    d.rtSetInt1(r, "sampler.spp", spp)
    d.rtSetFloat1(r, "tMaxShadowRay", 1e4)
    d.rtCommit(r)
    tm = d.rtNewToneMapper("default")
    d.rtCommit(tm)
    return r, cam, scene, tm


def _moving_mesh_arrays():
    """The moving quad of scenes/samples/sphere_motion.xml (the TriangleMesh with <motions>)."""
    src = (SCENES / "samples" / "sphere_motion.xml").read_text()
    mesh = next(m for m in re.findall(r"<TriangleMesh>.*?</TriangleMesh>", src, flags=re.S) if "<motions>" in m)
    def arr(tag, cols, dtype=F):
        return np.array(re.search(rf"<{tag}>(.*?)</{tag}>", mesh, flags=re.S).group(1).split(), dtype).reshape(-1, cols)
    return arr("positions", 3), arr("triangles", 3, np.int32), arr("normals", 3), arr("texcoords", 2), arr("motions", 3)


def _kinds_scene(d):
    """Every geometry kind, each in view; the `triangle` shape comes last, so its one triangle has
    the largest global id, and it lies under the centre of the image."""
    import denoise_albedo_ref as aref
    tex = aref.texture(d, "bilinear", aref.texture_image(8))
    uber_tex = aref.material(d, "Uber", [("diffuse", (0.8, 0.7, 0.6)), ("roughness", 0.25), ("eta", 1.5)],
                             textures=[("Kd", tex)])
    uber = aref.material(d, "Uber", [("diffuse", (0.3, 0.6, 0.4)), ("roughness", 0.0)])
    matte = aref.material(d, "Matte", [("reflectance", (0.7, 0.5, 0.3))])
    matte_tex = aref.material(d, "MatteTextured", textures=[("Kd", tex)])
    scene = d.rtNewScene("default")
    # a full mesh with normals and texture coordinates under a textured Uber material
    d.rtSetPrimitive(scene, 0, d.rtNewShapePrimitive(_mesh(d, _bent_quad(1), normals=_normals(1), uv=QUAD_UV), uber_tex,
                                                     _move(-125, 0, 110)))
    # a mesh with normals only (TriangleMeshWithNormals)
    d.rtSetPrimitive(scene, 1, d.rtNewShapePrimitive(_mesh(d, _bent_quad(2), normals=_normals(2)), matte,
                                                     _move(125, 0, 110)))
    # a full mesh with neither normals nor texture coordinates (TriangleMeshFull: no normals array)
    d.rtSetPrimitive(scene, 2, d.rtNewShapePrimitive(_mesh(d, _bent_quad(3)), uber, _move(-125, 0, -90)))
    # sphere_motion's moving quad: the indexed source, while its record slot is loaded all the same
    pos, idx, nor, uv, mot = _moving_mesh_arrays()
    d.rtSetPrimitive(scene, 3, d.rtNewShapePrimitive(_mesh(d, pos, idx, normals=nor, uv=uv, motions=mot), matte_tex,
                                                     _move(125, 0, -90, 0.3)))
    _lights(d, scene, 4)
    tri = d.rtNewShape("triangle")
    for n, v in (("v0", (-50, 5, -60)), ("v1", (0, 5, 60)), ("v2", (50, 5, -60))):
        d.rtSetFloat3(tri, n, *v)
    d.rtCommit(tri)
    d.rtSetPrimitive(scene, 6, d.rtNewShapePrimitive(tri, matte))
    return _finish(d, scene, 4, 4)


def _central_ray():
    e, t = np.array(EYE, np.float64), np.array(TARGET, np.float64)
    dr = (t - e) / np.linalg.norm(t - e)
    org4 = np.array([[*EYE, 0.0]], F)
    dir4 = np.array([[*dr, np.inf]], F)
    return org4, dir4


def _uber_scene(d):
    """Four Uber quads, one per specular branch of Uber::shade plus a textured one, and a fifth
    quad without a material."""
    import denoise_albedo_ref as aref
    tex = aref.texture(d, "bilinear", aref.texture_image(8))
    mats = [
        aref.material(d, "Uber", [("diffuse", (0.7, 0.3, 0.2)), ("reflectivity", 0.6), ("roughness", 0.4)]),  # layered: p[9] > 0
        aref.material(d, "Uber", [("diffuse", (0.2, 0.6, 0.3)), ("roughness", 0.0), ("eta", 1.7)]),           # specular: p[8] == 0
        aref.material(d, "Uber", [("diffuse", (0.3, 0.3, 0.8)), ("roughness", 0.2), ("eta", 1.3)]),           # microfacet
        aref.material(d, "Uber", [("diffuse", (0.9, 0.9, 0.9)), ("roughness", 0.35)], textures=[("Kd", tex)]),  # + Kd texture
        None,                                                                                                  # g.material < 0
    ]
    where = [(-125, 0, 110), (125, 0, 110), (-125, 0, -90), (125, 0, -90), (0, 0, 10)]
    scene = d.rtNewScene("default")
    for k, (m, at) in enumerate(zip(mats, where)):
        mesh = _mesh(d, _bent_quad(k) * F(0.8 if m is None else 1.0), normals=_normals(k), uv=QUAD_UV)
        d.rtSetPrimitive(scene, k, d.rtNewShapePrimitive(mesh, m, _move(*at)))
    _lights(d, scene, 5)
    return _finish(d, scene, 3, 4)


def _render(d, built, w):
    r, cam, scene, tm = built
    fb = d.rtNewFrameBuffer("RGB_FLOAT32", w, w)
    d.rtRenderFrame(r, cam, scene, tm, fb, 0)
    st = d.render_stats()
    return d.framebuffer_array(fb, w, w, "RGB_FLOAT32").copy(), (st["raysClosest"], st["raysShadow"])


# ----------------------------------------------------------------------------- the oracle side
def test_kinds_scene_oracle_side(host_device):
    """The scene is what test 1 needs: five geometries of the four kinds and flag sets, a moving
    one among them, the last triangle of the array under the central ray, and every geometry in
    view of the camera (its triangles are hit by camera rays)."""
    d = host_device
    r, cam, scene, _ = _kinds_scene(d)
    blob = d.export_frame(r, cam, scene)
    assert b"motions" in blob
    n = d.scene_info(scene)["numTriangles"]
    hit = oracle.trace(blob, *_central_ray())
    assert hit[0, 3:4].view(np.int32)[0] == n - 1
    g, p = d.triangle_ids(scene, n - 1)
    assert p == 0  # the `triangle` shape's only triangle
    org, dr = oracle.camera_rays(blob, np.array([[x + 0.5, y + 0.5] for y in range(48) for x in range(48)], F) / 48)
    org4 = np.concatenate([org, np.zeros((len(org), 1), F)], axis=1)
    dir4 = np.concatenate([dr, np.full((len(dr), 1), np.inf, F)], axis=1)
    tri = oracle.trace(blob, org4, dir4)[:, 3].view(np.int32)
    geoms = {d.triangle_ids(scene, int(t))[0] for t in np.unique(tri[tri >= 0])}
    assert len(geoms) >= 5 and g in geoms
    img, st = oracle.render(blob, 48, 48, 1.0)
    assert np.isfinite(img).all() and img.std() > 0 and st["raysShadow"] > 0


def test_uber_scene_oracle_side(host_device):
    d = host_device
    r, cam, scene, _ = _uber_scene(d)
    img, st = oracle.render(d.export_frame(r, cam, scene), 32, 32, 1.0)
    assert np.isfinite(img).all() and img.std() > 0 and st["raysClosest"] > 32 * 32 * 4


# ----------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_every_geometry_kind_matches_the_oracle(gpu_device):
    import torch
    d = gpu_device
    built = _kinds_scene(d)
    r, cam, scene, _ = built
    img, rays = _render(d, built, 48)
    ref, st = oracle.render(d.export_frame(r, cam, scene), 48, 48, 1.0)
    print("kinds:", (img != ref).sum(), "channels differ; rays", rays, (st["raysClosest"], st["raysShadow"]))
    parity(img, ref, 0.999, exact=True)
    assert rays == (st["raysClosest"], st["raysShadow"])
    # the record at the end of triShade is read: the central ray hits the last global triangle id
    org4, dir4 = _central_ray()
    o, dd = torch.from_numpy(org4).cuda(), torch.from_numpy(dir4).cuda()
    hit = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    d.intersect(scene, o.data_ptr(), dd.data_ptr(), 1, hit.data_ptr())
    assert hit.cpu().numpy()[0, 3:4].view(np.int32)[0] == d.scene_info(scene)["numTriangles"] - 1


@pytest.mark.gpu
def test_uber_branches_match_the_oracle(gpu_device):
    d = gpu_device
    built = _uber_scene(d)
    r, cam, scene, _ = built
    img, rays = _render(d, built, 32)
    ref, st = oracle.render(d.export_frame(r, cam, scene), 32, 32, 1.0)
    print("uber:", (img != ref).sum(), "channels differ; rays", rays, (st["raysClosest"], st["raysShadow"]))
    parity(img, ref, 0.999, exact=True)
    assert rays == (st["raysClosest"], st["raysShadow"])


C2 = c2_args(64, 4) + ["-depth", "4", "-fb", "RGB_FLOAT32"]


@pytest.fixture(scope="module")
def c2_default(gpu_device):
    """C2 at 64 x 64, 4 spp, depth 4 on the default device: frame, ray counts, oracle frame."""
    s = yrt.Session(C2, device=gpu_device)
    img = s.render().copy()
    st = gpu_device.render_stats()
    ref, ost = oracle.render(s.export_frame(), 64, 64, s.info()["gamma"])
    s.close()
    return img, (st["raysClosest"], st["raysShadow"]), ref, (ost["raysClosest"], ost["raysShadow"])


@pytest.mark.gpu
def test_two_direct_lights_match_the_oracle(c2_default):
    img, rays, ref, orays = c2_default
    print("c2:", (img != ref).sum(), "channels differ; rays", rays, orays)
    parity(img, ref, 0.999, exact=True)
    assert rays == orays and rays[1] > 0


@pytest.mark.gpu
def test_two_direct_lights_one_lane_and_split_batches(c2_default, monkeypatch):
    """Stores follow the reservations: no slot is written before it is reserved, whatever the
    lanes and however the frame is split into batches."""
    img, rays, _, _ = c2_default
    monkeypatch.setenv("YRT_LANES", "1")
    d = yrt.Device(0)
    try:
        out = []
        for cap in (0, 256 * 4 * 3, 256 * 4 * 5):  # one batch, 3 tiles and 5 tiles per batch
            if cap:
                d.set_batch_capacity(cap)
            s = yrt.Session(C2, device=d)
            out.append((s.render().copy(), d.render_stats()))
            s.close()
    finally:
        d.close()
    for o, st in out:
        assert np.array_equal(o, img)
        assert (st["raysClosest"], st["raysShadow"]) == rays
