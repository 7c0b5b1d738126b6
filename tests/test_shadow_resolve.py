"""The fused shadow resolve of k_trace<true> (csrc/kernels/k_trace.h, PathBuffers::fuseShadow: one
direct light): a shadow ray that ends unoccluded keeps its queue slot ("pending"), and its light
is added to its path's radiance at the wave's next refill or at the wave's end, not inside the
traversal loop. The sum is the same l + c per channel by one writer per path, so every frame
below equals its reference bit for bit.

1. every ray unoccluded, a wave's chunk at most 64: every lane is resolved at the wave's end;
2. every ray occluded: the kernel leaves the radiance alone;
3. mixed, more than 64 x YRT_TRACE_GRID queries in one launch: pending lanes resolved at refills,
   against the unfused path (YRT_NO_SHADOW_FUSE: sOcc + k_shadow_resolve);
4. NaN tfar (tMaxShadowRay infinite): a refilled ray with nothing to traverse goes pending;
5. two lights (C2): the unfused mode is what it was."""
import numpy as np
import pytest

import oracle
import yrt
from helpers import c2_args, parity
from test_shade_bursts import QUAD_IDX, _mesh, _render

F = np.float32
TRACE_GRID_QUERIES = 64 * 16384  # 64 x YRT_TRACE_GRID (yrt_kernels.h): above it a wave's chunk exceeds 64
BOX_IDX = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 4, 5], [0, 5, 1],
                    [1, 5, 6], [1, 6, 2], [2, 6, 7], [2, 7, 3], [3, 7, 4], [3, 4, 0]], np.int32)


def _quad(half, y=0.0):
    return np.array([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]], F)


def _box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return np.array([[x0, y0, z0], [x1, y0, z0], [x1, y0, z1], [x0, y0, z1],
                     [x0, y1, z0], [x1, y1, z0], [x1, y1, z1], [x0, y1, z1]], F)


def _box_grid(n=9, pitch=260.0, width=120.0, height=260.0):
    """n x n boxes standing on the ground about the origin, as one mesh."""
    pos, idx = [], []
    for i in range(n):
        for j in range(n):
            cx, cz = (i - (n - 1) / 2) * pitch, (j - (n - 1) / 2) * pitch
            idx.append(BOX_IDX + 8 * len(pos))
            pos.append(_box((cx - width / 2, 0.0, cz - width / 2), (cx + width / 2, height, cz + width / 2)))
    return np.concatenate(pos), np.concatenate(idx)


def _scene(d, meshes, eye, target, depth, spp, tmax=1e4):
    """The meshes under one matte material and one ambient light: one direct light, so the shadow
    resolve is fused into the any-hit trace."""
    import denoise_albedo_ref as aref
    from test_cpu_host import yrt_lookat
    matte = aref.material(d, "Matte", [("reflectance", (0.7, 0.5, 0.3))])
    scene = d.rtNewScene("default")
    for k, (pos, idx) in enumerate(meshes):
        d.rtSetPrimitive(scene, k, d.rtNewShapePrimitive(_mesh(d, pos, idx), matte))
    amb = d.rtNewLight("ambientlight")
    d.rtSetFloat3(amb, "L", 0.6, 0.7, 0.9)
    d.rtCommit(amb)
    d.rtSetPrimitive(scene, len(meshes), d.rtNewLightPrimitive(amb))
    d.rtCommit(scene)
    cam = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam, "local2world", yrt_lookat(eye, target, (0, 1, 0)))
    d.rtSetFloat1(cam, "angle", 60.0)
    d.rtSetFloat1(cam, "aspectRatio", 1.0)
    d.rtCommit(cam)
    r = d.rtNewRenderer("pathtracer")
    d.rtSetInt1(r, "maxDepth", depth)
    d.rtSetInt1(r, "sampler.spp", spp)
    d.rtSetFloat1(r, "tMaxShadowRay", tmax)
    d.rtCommit(r)
    tm = d.rtNewToneMapper("default")
    d.rtCommit(tm)
    return r, cam, scene, tm


DOWN = ((0.0, 600.0, -600.0), (0.0, 0.0, 0.0))  # 45 degrees down: every camera ray meets the ground


def _ground_scene(d, tmax=1e4):
    return _scene(d, [(_quad(6000.0), QUAD_IDX)], *DOWN, depth=3, spp=1, tmax=tmax)


def _closed_box_scene(d):
    eye = (0.0, 250.0, -420.0)
    return _scene(d, [(_box((-600, -100, -600), (600, 600, 600)), BOX_IDX)], eye, (0.0, 0.0, 0.0), depth=3, spp=1)


def _mixed_scene(d):
    return _scene(d, [(_quad(6000.0), QUAD_IDX), _box_grid()], *DOWN, depth=1, spp=2)


def _oracle(d, built, w):
    r, cam, scene, _ = built
    ref, st = oracle.render(d.export_frame(r, cam, scene), w, w, 1.0)
    return ref, (st["raysClosest"], st["raysShadow"])


# ----------------------------------------------------------------------------- the oracle side
def test_scenes_are_what_the_gpu_tests_need(host_device):
    """Ground alone: every pixel's one sample is lit (nothing can occlude a ray that leaves a flat
    ground upwards) and every path casts its shadow ray. Closed box: no light arrives at all, while
    shadow rays are cast. Mixed: of rays leaving the ground between the boxes upwards, a share
    well inside (0, 1) is occluded."""
    d = host_device
    img, rays = _oracle(d, _ground_scene(d), 40)
    assert (img > 0).all() and rays[1] >= 1600
    img, rays = _oracle(d, _ground_scene(d, tmax=float("inf")), 32)
    assert (img > 0).all() and rays[1] >= 1024
    img, rays = _oracle(d, _closed_box_scene(d), 32)
    assert (img == 0).all() and rays[1] >= 1024
    r, cam, scene, _ = _mixed_scene(d)
    rng = np.random.default_rng(7)
    n = 4096
    org = np.concatenate([rng.uniform(-1200, 1200, (n, 1)), np.full((n, 1), 0.01), rng.uniform(-1200, 1200, (n, 1)),
                          np.zeros((n, 1))], axis=1).astype(F)
    u, phi = rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)  # cosine-weighted about +y
    s = np.sqrt(1 - u)
    dr = np.stack([s * np.cos(phi), np.sqrt(u), s * np.sin(phi), np.full(n, 1e4)], axis=1).astype(F)
    occ = oracle.trace(d.export_frame(r, cam, scene), org, dr, any_hit=True)[:, 3].view(np.int32) != 0  # 0 / 1 flags
    print("mixed: occluded share of upward rays from the ground", occ.mean())
    assert 0.25 < occ.mean() < 0.75


# ----------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_every_ray_unoccluded_resolved_at_the_waves_end(gpu_device):
    """1 600 paths, not a multiple of 64, in chunks of at most 64: no wave refills with a pending
    lane, every contribution is added on the way out."""
    d = gpu_device
    built = _ground_scene(d)
    img, rays = _render(d, built, 40)
    ref, orays = _oracle(d, built, 40)
    print("unoccluded:", (img != ref).sum(), "channels differ; rays", rays, orays)
    parity(img, ref, 0.999, exact=True)
    assert rays == orays and rays[1] >= 1600


@pytest.mark.gpu
def test_every_ray_occluded_leaves_the_radiance_alone(gpu_device):
    d = gpu_device
    built = _closed_box_scene(d)
    img, rays = _render(d, built, 32)
    ref, orays = _oracle(d, built, 32)
    print("occluded:", (img != ref).sum(), "channels differ; rays", rays, orays)
    parity(img, ref, 0.999, exact=True)
    assert rays == orays and rays[1] > 0


@pytest.mark.gpu
def test_mixed_rays_resolved_at_refills_equal_the_unfused_path(monkeypatch):
    """More than 64 x YRT_TRACE_GRID shadow queries in one launch: chunks above 64, so waves refill
    with pending lanes. The reference is the same render through sOcc and k_shadow_resolve."""
    monkeypatch.setenv("YRT_LANES", "1")
    monkeypatch.delenv("YRT_NO_SHADOW_FUSE", raising=False)
    d = yrt.Device(0)
    try:
        built = _mixed_scene(d)
        fused, rays = _render(d, built, 1024)
        monkeypatch.setenv("YRT_NO_SHADOW_FUSE", "1")
        unfused, urays = _render(d, built, 1024)
    finally:
        d.close()
    print("mixed:", (fused != unfused).sum(), "channels differ; rays", rays, urays,
          "black share", (fused == 0).all(axis=2).mean())
    assert rays[1] > TRACE_GRID_QUERIES, rays
    assert rays == urays
    assert np.isfinite(fused).all() and fused.std() > 0
    assert fused.tobytes() == unfused.tobytes()


@pytest.mark.gpu
def test_nan_tfar_rays_go_pending(gpu_device, monkeypatch):
    """tMaxShadowRay infinite: tfar is NaN, the ray has nothing to traverse and is unoccluded."""
    d = gpu_device
    built = _ground_scene(d, tmax=float("inf"))
    monkeypatch.delenv("YRT_NO_SHADOW_FUSE", raising=False)
    fused, rays = _render(d, built, 32)
    monkeypatch.setenv("YRT_NO_SHADOW_FUSE", "1")
    unfused, urays = _render(d, built, 32)
    ref, orays = _oracle(d, built, 32)
    print("nan tfar:", (fused != ref).sum(), (unfused != ref).sum(), "channels differ; rays", rays, urays, orays)
    assert fused.tobytes() == unfused.tobytes() and rays == urays
    parity(fused, ref, 0.999, exact=True)
    parity(unfused, ref, 0.999, exact=True)
    assert rays == orays and rays[1] >= 1024


@pytest.mark.gpu
def test_two_lights_keep_the_unfused_path(gpu_device, monkeypatch):
    """C2 has two lights: occlusion flags and k_shadow_resolve, untouched by the deferred resolve."""
    monkeypatch.delenv("YRT_ALL_DIRECT_LIGHTS", raising=False)
    s = yrt.Session(c2_args(64, 4) + ["-depth", "4", "-fb", "RGB_FLOAT32"], device=gpu_device)
    try:
        img = s.render().copy()
        st = gpu_device.render_stats()
        ref, ost = oracle.render(s.export_frame(), 64, 64, s.info()["gamma"])
    finally:
        s.close()
    rays, orays = (st["raysClosest"], st["raysShadow"]), (ost["raysClosest"], ost["raysShadow"])
    print("c2:", (img != ref).sum(), "channels differ; rays", rays, orays)
    parity(img, ref, 0.999, exact=True)
    assert rays == orays and rays[1] > 0
