"""The denoise stage: first-hit guide buffers (yrtRenderGuides), the edge-avoiding
a-trous filter (yrtDenoiseFrameBuffer) and the tone mapper's vignette, against the float64 numpy
restatement of tests/denoise_ref.py; the CPU tests cover the refusals, the parameter struct's size
rule and the front end's -denoise tag."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import yrt
from yrt import _native as N

import denoise_ref as ref
from denoise_albedo_ref import mapped, pixels, reldev
from helpers import c1_args
from trace_scenes import MeshScene

W, H = 40, 24          # not a multiple of the 16-pixel tile
W8 = 38                # 3 * 38 = 114 bytes per RGB8 row, padded to 116
FORMATS = ("RGB8", "RGBA8", "RGB_FLOAT32", "RGBA_FLOAT32")
DEFAULTS = dict(sigma_color=1.0, sigma_normal=64.0, sigma_position=float(np.float32(0.02)))  # the library's floats

# Largest relative deviation |gpu - numpy| / max(|numpy|, 1/255) of the float filter measured on an
# MI355X over the cases below: 4.5e-7, 8.7e-7 and 8.6e-7 for 1, 3 and 5 iterations (either float
# format), 1.17e-6 and 8.0e-7 for the two cube faces. The bound is 8x the largest, far below the
# 1e-4 ceiling (float32 epsilon x 25 taps x 5 iterations x the exponent 64 of the normal weight).
FILTER_MEASURED = 1.17e-6
FILTER_BOUND = min(8 * FILTER_MEASURED, 1e-4)


class Quads:
    """The two-quad scene under an emissive triangle, a 4-spp depth-2 path tracer and a default tone
    mapper; frames and guides are rendered once per (format, size) and shared."""

    def __init__(self, dev):
        self.dev = dev
        self.ms = MeshScene(dev, ref.two_quads(), eye=(0, 0, 0), look=(0, 0, 1), up=(0, 1, 0), angle=60.0)
        ref.add_triangle_light(self.ms)
        self.renderer = dev.rtNewRenderer("pathtracer")
        dev.rtSetInt1(self.renderer, "maxDepth", 2)
        dev.rtSetInt1(self.renderer, "sampler.spp", 4)
        dev.rtCommit(self.renderer)
        self.tm = dev.rtNewToneMapper("default")
        dev.rtCommit(self.tm)
        self._raw, self._guides = {}, {}

    def render(self, fmt, w=W, h=H):
        """A fresh framebuffer holding the frame, not mapped yet."""
        fb = self.dev.rtNewFrameBuffer(fmt, w, h)
        self.dev.rtRenderFrame(self.renderer, self.ms.camera, self.ms.scene, self.tm, fb, 0)
        return fb

    def raw(self, fmt, w=W, h=H):
        if (fmt, w, h) not in self._raw:
            self._raw[fmt, w, h] = mapped(self.dev, self.render(fmt, w, h), fmt, w, h)
        return self._raw[fmt, w, h]

    def guides(self, w=W, h=H):
        if (w, h) not in self._guides:
            self._guides[w, h] = self.dev.render_guides(self.ms.camera, self.ms.scene, w, h)
        return self._guides[w, h]

    def denoised(self, fmt, w=W, h=H, **kw):
        fb = self.render(fmt, w, h)
        self.dev.denoise(self.ms.camera, self.ms.scene, fb, **kw)
        return mapped(self.dev, fb, fmt, w, h)

    def expect(self, fmt, w=W, h=H, iterations=5):
        """The numpy filter on the GPU's own undenoised frame and guides: (h, w, 3) float64."""
        px = pixels(self.raw(fmt, w, h), fmt, w)[..., :3]
        c0 = px.astype(np.float64) / 255.0 if px.dtype == np.uint8 else px.astype(np.float64)
        pos, nrm = self.guides(w, h)
        return ref.atrous(c0, pos, nrm, iterations, **DEFAULTS)


@pytest.fixture(scope="module")
def quads(gpu_device):
    return Quads(gpu_device)


# ----------------------------------------------------------------------------- CPU
def test_host_device_refuses_guides_and_denoise(host_device):
    ms = MeshScene(host_device, ref.two_quads(), eye=(0, 0, 0), look=(0, 0, 1))
    fb = host_device.rtNewFrameBuffer("RGB_FLOAT32", 8, 8)
    with pytest.raises(RuntimeError, match="host-only"):
        host_device.render_guides(ms.camera, ms.scene, 8, 8)
    with pytest.raises(RuntimeError, match="host-only"):
        host_device.denoise(ms.camera, ms.scene, fb)


def test_denoise_params_size_is_checked(host_device):
    ms = MeshScene(host_device, ref.two_quads(), eye=(0, 0, 0), look=(0, 0, 1))
    fb = host_device.rtNewFrameBuffer("RGB_FLOAT32", 8, 8)
    p = N.DenoiseParams(size=2, iterations=1)
    assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
    assert "size" in host_device.error() and "host-only" not in host_device.error()
    # a struct that ends after `iterations` is accepted (the call then fails on the host-only device)
    p = N.DenoiseParams(size=8, iterations=1, sigmaNormal=-1.0)  # sigmaNormal lies beyond size: not read
    assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
    assert "host-only" in host_device.error()
    # and a full-size struct's fields are read: a negative sigmaNormal is refused
    p = N.DenoiseParams(size=C.sizeof(N.DenoiseParams), iterations=1, sigmaColor=1, sigmaNormal=-1.0, sigmaPosition=1)
    assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
    assert "sigmaNormal" in host_device.error()
    # defaults: filled up to the caller's size only
    p = N.DenoiseParams(size=12, iterations=-7, sigmaColor=-7, sigmaNormal=-7, sigmaPosition=-7)
    assert N.dev.yrtDenoiseDefaults(C.byref(p)) == 0
    assert (p.iterations, p.sigmaColor, p.sigmaNormal, p.sigmaPosition) == (5, 1.0, -7, -7)
    assert yrt.Device.denoise_defaults() == dict(iterations=5, **DEFAULTS)
    p = N.DenoiseParams(size=3)
    assert N.dev.yrtDenoiseDefaults(C.byref(p)) != 0


def test_vignetting_commits(host_device):
    tm = host_device.rtNewToneMapper("default")
    host_device.rtSetBool1(tm, "vignetting", True)
    host_device.rtCommit(tm)


def test_denoise_tag_parses(host_device):
    yrt.Session(c1_args(16) + ["-denoise", "3"], device=host_device).close()
    yrt.Session(c1_args(16) + ["-denoise", "0"], device=host_device).close()
    with pytest.raises(RuntimeError, match="-denoise"):
        yrt.Session(c1_args(16) + ["-denoise", "-1"], device=host_device)


# ----------------------------------------------------------------------------- GPU, guides
@pytest.mark.gpu
def test_guides_match_pick(quads):
    """pos4.xyz = rtPick at the pixel centre (at most 2 ulp of the largest coordinate: two kernels
    may contract multiply-adds differently) and t |dir| = |pos - org| within the same bound."""
    import oracle
    d, ms = quads.dev, quads.ms
    pos, nrm = quads.guides()
    fx = (np.arange(W, dtype=np.float32) + np.float32(0.5)) / np.float32(W)
    fy = (np.arange(H, dtype=np.float32) + np.float32(0.5)) / np.float32(H)
    px = np.stack(np.meshgrid(fx, fy), -1).reshape(-1, 2)
    org, dr = oracle.camera_rays(ms.blob, px)
    dlen = np.linalg.norm(dr.astype(np.float64), axis=1).reshape(H, W)
    worst = worst_t = 0.0
    hits = 0
    for y in range(H):
        for x in range(W):
            hit, p = d.rtPick(ms.camera, fx[x], fy[y], ms.scene)
            assert hit == bool(np.isfinite(pos[y, x, 3])), (x, y)
            if not hit:
                continue
            hits += 1
            g = pos[y, x, :3]
            ulp = float(np.spacing(np.abs(g).max()))
            worst = max(worst, float(np.abs(g.astype(np.float64) - np.asarray(p, np.float64)).max()) / ulp)
            dist = np.linalg.norm(g.astype(np.float64) - org[y * W + x])
            worst_t = max(worst_t, abs(float(pos[y, x, 3]) * dlen[y, x] - dist) / ulp)
    print(f"guides vs rtPick: {hits} hits, worst position {worst} ulp, worst t {worst_t} ulp")
    assert 0 < hits < W * H
    assert worst <= 2 and worst_t <= 2


@pytest.mark.gpu
def test_guide_normals_and_misses(quads):
    """Flat quads: nrm4.xyz is the quad's analytic normal towards the camera within one normalize:
    the edge cross product is exact (dyadic coordinates), rsqrt is within 4 ulp (test_sse_rcp.py),
    the product adds half an ulp and the float64 reference another half: 5 * 2^-23 relative."""
    pos, nrm = quads.guides()
    hit = np.isfinite(pos[..., 3])
    near = hit & (np.abs(pos[..., 2] - ref.QUAD_NEAR_Z) < 1e-3)  # the other quad lies at z >= 3
    tilt = hit & ~near
    assert near.sum() > 50 and tilt.sum() > 50 and (~hit).sum() > 50
    tol = 5 * 2.0 ** -23
    assert np.abs(nrm[near][:, :3] - ref.N_NEAR).max() <= tol
    assert np.abs(nrm[tilt][:, :3] - ref.N_TILT).max() <= tol
    assert np.all(nrm[hit][:, 3] == 1)
    # the tilted quad's points lie on its plane x + z = 5, between depth 3 and 5
    assert np.abs(pos[tilt][:, 0] + pos[tilt][:, 2] - 5).max() < 1e-5
    miss = ~hit
    assert np.array_equal(pos[miss], np.broadcast_to(np.float32([0, 0, 0, np.inf]), pos[miss].shape))
    assert np.array_equal(nrm[miss], np.zeros_like(nrm[miss]))
    assert not np.signbit(pos[miss][:, :3]).any() and not np.signbit(nrm[miss]).any()


@pytest.mark.gpu
def test_guide_normals_interpolate(gpu_device):
    """The reference's sphere (numTheta 8, numPhi 16, vertex normals) seen from its equator, both
    polar caps out of view. The guide normal has unit length, faces the viewer and agrees with
    (p - centre) / r to the tessellation's error E, computed from the mesh: the largest
    |Ns(b) - (p(b) - c) / r| over a 33 x 33 barycentric lattice of every non-polar triangle, plus
    what both sides can change over half a lattice step (each at most edge / r per unit of b), plus
    the float32 noise of the vertex normals' forward differences (4 ulp of 1 over the smallest
    difference vector, per operand of the cross product) and 2e-6 for the hit point and the
    interpolation in float32."""
    from test_cpu_host import yrt_lookat
    d = gpu_device
    nt, nphi, r, dist = 8, 16, 1.0, 1.6
    sph = d.rtNewShape("sphere")
    d.rtSetFloat3(sph, "P", 0.0, 0.0, 0.0)
    d.rtSetFloat1(sph, "r", r)
    d.rtSetInt1(sph, "numTheta", nt)
    d.rtSetInt1(sph, "numPhi", nphi)
    d.rtCommit(sph)
    mat = d.rtNewMaterial("Matte")
    d.rtCommit(mat)
    scene = d.rtNewScene("default")
    d.rtSetPrimitive(scene, 0, d.rtNewShapePrimitive(sph, mat))
    d.rtCommit(scene)
    cam = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam, "local2world", yrt_lookat((0, 0, -dist), (0, 0, 0), (0, 1, 0)))
    d.rtSetFloat1(cam, "angle", 40.0)
    d.rtSetFloat1(cam, "aspectRatio", 1.0)
    d.rtCommit(cam)
    pos, nrm = d.render_guides(cam, scene, W, H)
    hit = np.isfinite(pos[..., 3])
    assert hit.sum() > W * H // 2
    p, n = pos[hit][:, :3].astype(np.float64), nrm[hit][:, :3].astype(np.float64)
    # visible points lie below the latitude acos(r / dist) = 51.3 degrees; the polar triangles start at 67.5
    assert np.abs(p[:, 1]).max() < r * np.cos(np.pi / nt) * 0.95
    # unit length: rsqrt within 4 ulp, the dot product's three products and two sums, the scaling
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 8 * 2.0 ** -23
    assert ((n * (p - np.array([0, 0, -dist]))).sum(1) < 0).all()

    vp, vn, tris, sin_t = ref.sphere_mesh(nt, nphi, r)
    polar = (tris < nphi).any(1) | (tris >= nt * nphi).any(1)
    tris = tris[~polar]
    k = 32
    b1, b2 = np.meshgrid(np.arange(k + 1) / k, np.arange(k + 1) / k)
    keep = b1 + b2 <= 1 + 1e-12
    b1, b2 = b1[keep], b2[keep]
    b0 = 1 - b1 - b2
    P = b0[None, :, None] * vp[tris[:, 0]][:, None] + b1[None, :, None] * vp[tris[:, 1]][:, None] + \
        b2[None, :, None] * vp[tris[:, 2]][:, None]
    Ns = b0[None, :, None] * vn[tris[:, 0]][:, None] + b1[None, :, None] * vn[tris[:, 1]][:, None] + \
        b2[None, :, None] * vn[tris[:, 2]][:, None]
    Ns /= np.linalg.norm(Ns, axis=-1, keepdims=True)
    lattice = np.abs(Ns - P / r).max()
    edge = max(np.linalg.norm(vp[tris[:, a]] - vp[tris[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    used = np.unique(tris)
    step = 0.001 * min(np.pi / nt, 2 * np.pi / nphi * sin_t[used].min())  # the smallest difference vector
    E = lattice + 2 * (edge / r) / (2 * k) + 2 * (4 * 2.0 ** -23 / step) + 2e-6
    dev = np.abs(n - p / r).max()
    print(f"sphere normals: deviation {dev:.4g}, tessellation error {E:.4g} (lattice {lattice:.4g})")
    assert dev <= E
    assert E < 0.1  # the bound itself stays a tessellation-sized number


# ----------------------------------------------------------------------------- GPU, filter
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_matches_numpy(quads, fmt, iterations):
    """Measured on an MI355X: 4.5e-7, 8.7e-7, 8.6e-7 for 1, 3, 5 iterations (FILTER_MEASURED). Step
    16 of the fifth iteration sends taps outside the 40 x 24 frame on every side."""
    raw = pixels(quads.raw(fmt), fmt, W)
    assert (raw[..., :3].max(-1) > 0.01).mean() > 0.2, "the scene must be lit"
    got = pixels(quads.denoised(fmt, iterations=iterations), fmt, W)
    want = quads.expect(fmt, iterations=iterations)
    hit = np.isfinite(quads.guides()[0][..., 3])
    dev = reldev(got[..., :3][hit], want[hit])
    print(f"filter {fmt} x{iterations}: relative deviation {dev:.3g}")
    assert np.abs(got[..., :3][hit].astype(np.float64) - raw[..., :3][hit]).max() > 1e-3, "the filter must act"
    assert dev <= FILTER_BOUND
    assert np.array_equal(got[~hit].view(np.uint32), raw[~hit].view(np.uint32))
    if fmt == "RGBA_FLOAT32":
        assert np.array_equal(got[..., 3], raw[..., 3])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB8", "RGBA8"])
def test_filter_8bit(quads, fmt):
    """Bytes within 1 of the numpy result quantized the same way; alpha, the padded bytes of the
    RGB8 rows (width 38: 114 of 116 bytes) and the miss pixels are untouched."""
    d = quads.dev
    fb = quads.render(fmt, W8, H)
    raw = mapped(d, fb, fmt, W8, H)
    if fmt == "RGB8":  # mark the padding, so that a store into it shows
        raw[:, 3 * W8:] = 0xA5
        mapped(d, fb, fmt, W8, H, write=raw)
    assert np.array_equal(raw, mapped(d, fb, fmt, W8, H))
    d.denoise(quads.ms.camera, quads.ms.scene, fb)
    out = mapped(d, fb, fmt, W8, H)
    got, before = pixels(out, fmt, W8), pixels(raw, fmt, W8)
    assert np.array_equal(pixels(quads.raw(fmt, W8, H), fmt, W8), before)
    want = ref.quantize(quads.expect(fmt, W8, H))
    hit = np.isfinite(quads.guides(W8, H)[0][..., 3])
    diff = np.abs(got[..., :3][hit].astype(int) - want[hit].astype(int))
    print(f"filter {fmt}: {float((diff > 0).mean()):.4f} of the bytes differ by 1, max {diff.max()}")
    assert diff.max() <= 1
    assert (got[..., :3][hit] != before[..., :3][hit]).mean() > 0.2, "the filter must act"
    assert np.array_equal(got[~hit], before[~hit])
    if fmt == "RGBA8":
        assert np.array_equal(got[..., 3], before[..., 3])
    else:
        assert np.all(out[:, 3 * W8:] == 0xA5)
    # the frame filtered where it was rendered (RGB8: in HBM) holds the same pixels
    assert np.array_equal(pixels(quads.denoised(fmt, W8, H), fmt, W8), got)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_zero_iterations_write_nothing(quads, fmt):
    w = W8 if fmt == "RGB8" else W
    fb = quads.render(fmt, w, H)
    raw = mapped(quads.dev, fb, fmt, w, H)
    quads.dev.denoise(quads.ms.camera, quads.ms.scene, fb, iterations=0)
    assert np.array_equal(mapped(quads.dev, fb, fmt, w, H), raw)
    # and on a frame not mapped yet (the RGB8 padding of a frame in HBM is whatever the block held)
    assert np.array_equal(pixels(quads.denoised(fmt, w, H, iterations=0), fmt, w), pixels(raw, fmt, w))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
def test_constant_frame_is_kept(quads, fmt):
    """An uploaded frame whose hit pixels all hold one value: the weights normalize, so every hit
    pixel keeps it (2 ulp), whatever the misses hold."""
    d = quads.dev
    fb = quads.render(fmt)
    hit = np.isfinite(quads.guides()[0][..., 3])
    value = np.float32([0.7231, 0.05, 3.5])
    px = pixels(mapped(d, fb, fmt, W, H), fmt, W).copy()
    px[..., :3] = np.float32(9.0)
    px[hit, :3] = value
    mapped(d, fb, fmt, W, H, write=px.view(np.uint8).reshape(H, -1))
    d.denoise(quads.ms.camera, quads.ms.scene, fb)
    out = pixels(mapped(d, fb, fmt, W, H), fmt, W)
    assert np.all(np.abs(out[hit][:, :3] - value) <= 2 * np.spacing(value))
    assert np.array_equal(out[~hit], px[~hit])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_is_filtered_where_it_lives(quads, fmt):
    """Denoised before the first map, or mapped, unmapped and then denoised: the same pixels, and
    the second map returns the filtered frame."""
    w = W8 if fmt == "RGB8" else W
    d = quads.dev
    first = pixels(quads.denoised(fmt, w, H), fmt, w)
    fb = quads.render(fmt, w, H)
    raw = pixels(mapped(d, fb, fmt, w, H), fmt, w)
    d.denoise(quads.ms.camera, quads.ms.scene, fb)
    second = pixels(mapped(d, fb, fmt, w, H), fmt, w)
    assert not np.array_equal(second, raw)
    assert np.array_equal(first.view(np.uint8), second.view(np.uint8))


@pytest.mark.gpu
def test_cube_job_faces(quads):
    """Two frames of one rtRenderFrames job (the second seen from the side), each denoised through
    its own camera while both still lie in the job's frame block."""
    from test_cpu_host import yrt_lookat
    d, ms, S = quads.dev, quads.ms, 32
    cam2 = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam2, "local2world", yrt_lookat((-1.5, 0.3, 0.5), (0.5, 0, 3.5), (0, 1, 0)))
    d.rtSetFloat1(cam2, "angle", 70.0)
    d.rtSetFloat1(cam2, "aspectRatio", 1.0)
    d.rtCommit(cam2)
    cams = [ms.camera, cam2]

    def job():
        fbs = [d.rtNewFrameBuffer("RGB_FLOAT32", S, S) for _ in cams]
        d.rtRenderFrames(quads.renderer, cams, ms.scene, quads.tm, fbs, 0)
        return fbs

    raws = [d.framebuffer_array(fb, S, S, "RGB_FLOAT32") for fb in job()]
    fbs = job()
    for fb, cam in zip(fbs, cams):
        d.denoise(cam, ms.scene, fb, iterations=3)
    assert not np.array_equal(raws[0], raws[1])
    for fb, cam, raw in zip(fbs, cams, raws):
        got = d.framebuffer_array(fb, S, S, "RGB_FLOAT32")
        pos, nrm = d.render_guides(cam, ms.scene, S, S)
        hit = np.isfinite(pos[..., 3])
        assert 50 < hit.sum() < S * S
        want = ref.atrous(raw, pos, nrm, 3, **DEFAULTS)
        dev = reldev(got[hit], want[hit])
        print(f"cube face: relative deviation {dev:.3g}")
        assert dev <= FILTER_BOUND
        assert np.array_equal(got[~hit], raw[~hit]) and not np.array_equal(got[hit], raw[hit])


# ----------------------------------------------------------------------------- GPU, vignette
@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [1.0, 2.2])
def test_vignetting(gpu_device, gamma):
    """frame(vignetting) = frame x cos(d / 2)^3, after the gamma. Relative tolerance, in units of
    2^-23 (one float32 ulp, relative): rcp(W / 2) <= 2 (test_sse_rcp.py), so v = (x - W/2) rcp <= 2.5,
    v^2 <= 5.5, the sum <= 6, the square root <= 3.5 = the error of the cosine's argument a = d / 2
    <= 0.708; through the cosine |tan a| a 3.5 <= 2.1, plus cosf's own 3 (test_libm.py): 5.1; cubed
    by powf: 3 x 5.1 = 15.3, i.e. 1.83e-6, plus powf's own 2e-5 (test_libm.py) and half an ulp for
    the product with the colour: 2.19e-5."""
    S = 16
    tol = 2e-5 + 15.3 * 2.0 ** -23 + 2.0 ** -24

    def frame(*extra):
        s = yrt.Session(c1_args(S, 4) + ["-fb", "RGB_FLOAT32", "-gamma", str(gamma)] + list(extra), device=gpu_device)
        img = s.render()
        s.close()
        return img.astype(np.float64)

    plain, vig = frame(), frame("-vignetting", "1")
    f = ref.vignette(S, S)[..., None]
    assert plain.max() > 0.1 and f.min() < 0.5 and f.max() == 1.0
    want = plain * f
    err = np.abs(vig - want) / np.maximum(want, 1e-30)
    print(f"vignetting gamma {gamma}: relative error {err.max():.3g} (tolerance {tol:.3g})")
    assert (np.abs(vig - want) <= tol * want).all()
    if gamma != 1.0:
        # the other order, (linear x factor)^(1/gamma), is a different frame
        other = (plain ** gamma * f) ** (1 / gamma)
        lit = want > 1e-3
        assert (np.abs(vig - other)[lit] > 100 * tol * want[lit]).mean() > 0.5


# ----------------------------------------------------------------------------- GPU, it denoises
@pytest.mark.gpu
def test_denoised_frame_is_closer_to_the_converged_one(gpu_device):
    """C1 at 64 x 64: the 4-spp frame filtered with the default parameters has a strictly lower mean
    squared error against the 1024-spp frame than the raw 4-spp frame (CPU rehearsal with the
    oracle's frames and the numpy filter: ratio 0.993 over the whole frame, which the emitter's
    pixels dominate; 0.28 over the pixels below 1)."""
    S = 64
    d = gpu_device

    def session(spp):
        return yrt.Session(c1_args(S, spp) + ["-fb", "RGB_FLOAT32"], device=d)

    s = session(1024)
    conv = s.render().astype(np.float64)
    s.close()
    s = session(4)
    raw = s.render().astype(np.float64)
    i = s.info()
    s.render(read=False)
    d.denoise(s.camera(), i["scene"], i["framebuffer"])
    den = d.framebuffer_array(i["framebuffer"], S, S, "RGB_FLOAT32").astype(np.float64)
    s.close()
    s = yrt.Session(c1_args(S, 4) + ["-fb", "RGB_FLOAT32", "-denoise", "5"], device=d)
    tagged = s.render().astype(np.float64)
    s.close()
    mse_raw, mse_den = ((raw - conv) ** 2).mean(), ((den - conv) ** 2).mean()
    dark = (conv.max(-1) < 1) & (raw.max(-1) < 1)
    print(f"C1 64x64: mse raw {mse_raw:.6g} denoised {mse_den:.6g} ratio {mse_den / mse_raw:.4f}; pixels below 1: "
          f"ratio {((den - conv)[dark] ** 2).mean() / ((raw - conv)[dark] ** 2).mean():.4f}")
    assert mse_den < mse_raw
    assert np.array_equal(tagged, den), "-denoise 5 is the default filter after the render"
