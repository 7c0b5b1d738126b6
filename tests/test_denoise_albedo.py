"""The texture-preserving denoise path: the first-hit albedo guide (yrtRenderAlbedo)
and the demodulated a-trous filter (YRTDenoiseParams::demodulate), against the numpy restatements
of tests/denoise_albedo_ref.py and tests/denoise_ref.py; the CPU tests cover the refusal, the
grown parameter struct's size rule, the binding's defaults and the front end's -denoise-albedo tag."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import yrt
from yrt import _native as N

import denoise_albedo_ref as aref
import denoise_ref as ref
from denoise_albedo_ref import mapped, pixels, reldev
from helpers import c1_args

W, H = 40, 24          # not a multiple of the 16-pixel tile
W8 = 38                # 3 * 38 = 114 bytes per RGB8 row, padded to 116
FORMATS = ("RGB8", "RGBA8", "RGB_FLOAT32", "RGBA_FLOAT32")
DEFAULTS = dict(sigma_color=1.0, sigma_normal=64.0, sigma_position=float(np.float32(0.02)))  # the library's floats
FLOOR = float(np.float32(1 / 255))
POWER = 1 / 2.2        # what a caller passes for a gamma-2.2 tone mapper
OLD_SIZE = 20          # sizeof(YRTDenoiseParams) before the demodulation fields

# The plain filter's derived ceiling (tests/test_denoise.py: float32 epsilon x 25 taps x 5 iterations x
# the exponent 64 of the normal weight) plus yrt_powf's 2e-5 (tests/test_libm.py) twice, for the
# demodulation and the remodulation. Not tightened to the measurement (see the tests' docstrings).
DEMOD_BOUND = 1e-4 + 2 * 2e-5

MATTE_A, MATTE_B = (0.2, 0.5, 0.8), (0.9, 0.1, 0.4)

# Error of a hit's (s, t), device against numpy, on the quads of aref.textured_quads (|P| <= 5.5, the
# camera at the origin). numpy side: P = t dir has two roundings, 2^-23 |P| <= 6.6e-7, over edges >= 1.
# Device side: the barycentrics are Moeller-Trumbore's U / den with U = dot(cross(dir, C), e) and
# den = dot(Ng, dir): six roundings each of terms bounded by |dir| |C| |e|, relative to |den| -- at
# most 1.15 x 2.3 x 1 / 1 on the near quad and 1.15 x 5.5 x 2.83 / 4 on the tilted one, i.e.
# 6 x 2^-24 x 4.5 = 1.6e-6 -- and three more roundings in w st0 + u st1 + v st2 (1.8e-7). Sum 2.5e-6.
ST_ERR = 2.5e-6


# ----------------------------------------------------------------------------- scenes
def _matte(dev, r):
    return aref.material(dev, "Matte", [("reflectance", r)])


class Plain:
    """denoise_ref's two quads with one Matte reflectance each."""

    def __init__(self, dev):
        (near, _, _), (tilt, _, _) = ref.two_quads()
        self.ms = aref.MaterialScene(dev, [(near, _matte(dev, MATTE_A)), (tilt, _matte(dev, MATTE_B))])
        self.pos, self.nrm = dev.render_guides(self.ms.camera, self.ms.scene, W, H)
        self.albedo = dev.render_albedo(self.ms.camera, self.ms.scene, W, H)


OBJ_KD = (0.5, 0.25, 0.75)
LIGHT_Z = 6.0


class Special:
    """The same two quads: the near one an Obj material with a map_Kd and a bump map whose texels
    (3/4, 1/4, 1/4) turn the shading normal round (b = 2 c - 1 = (1/2, -1/2, -1/2): without tangents
    normalize(b.z Ns) = -Ns), the tilted one a Mirror, and a triangle light in view above the near
    quad, on the plane z = 6."""

    def __init__(self, dev):
        (near, _, _), (tilt, _, _) = ref.two_quads()
        self.kd_image = aref.texture_image(4)
        bump = np.broadcast_to(np.float32([0.75, 0.25, 0.25]), (4, 4, 3)).copy()
        obj = aref.material(dev, "Obj", [("Kd", OBJ_KD)],
                            [("map_Kd", aref.texture(dev, "nearest", self.kd_image)),
                             ("map_Bump", aref.texture(dev, "nearest", bump))])
        mirror = aref.material(dev, "Mirror", [("reflectance", (0.9, 0.9, 0.9))])
        self.ms = aref.MaterialScene(dev, [(near, obj), (tilt, mirror)])
        ref.add_triangle_light(self.ms, v0=(-2.5, 1.8, LIGHT_Z), v1=(-1.5, 3.2, LIGHT_Z), v2=(-0.5, 1.8, LIGHT_Z))


class Textured:
    """aref.textured_quads: the near quad MatteTextured over an 8 x 8 image through a `nearest`
    texture, the tilted one over a 4 x 4 image through a `bilinear` one, under denoise_ref's triangle
    light; a 4-spp depth-2 path tracer and a default tone mapper. Frames, guides and albedo are
    rendered once per (format, size) and shared."""

    def __init__(self, dev):
        self.dev = dev
        self.img_near, self.img_tilt = aref.texture_image(8), aref.texture_image(4)
        near, tilt = aref.textured_quads()
        mats = [aref.material(dev, "MatteTextured", textures=[("Kd", aref.texture(dev, kind, img))])
                for kind, img in (("nearest", self.img_near), ("bilinear", self.img_tilt))]
        self.ms = aref.MaterialScene(dev, [(near, mats[0]), (tilt, mats[1])])
        ref.add_triangle_light(self.ms)
        self.renderer = dev.rtNewRenderer("pathtracer")
        dev.rtSetInt1(self.renderer, "maxDepth", 2)
        dev.rtSetInt1(self.renderer, "sampler.spp", 4)
        dev.rtCommit(self.renderer)
        self.tm = dev.rtNewToneMapper("default")
        dev.rtCommit(self.tm)
        self._raw, self._guides = {}, {}

    def render(self, fmt, w=W, h=H):
        fb = self.dev.rtNewFrameBuffer(fmt, w, h)
        self.dev.rtRenderFrame(self.renderer, self.ms.camera, self.ms.scene, self.tm, fb, 0)
        return fb

    def raw(self, fmt, w=W, h=H):
        if (fmt, w, h) not in self._raw:
            self._raw[fmt, w, h] = mapped(self.dev, self.render(fmt, w, h), fmt, w, h)
        return self._raw[fmt, w, h]

    def guides(self, w=W, h=H):
        """(pos4, nrm4, albedo4)"""
        if (w, h) not in self._guides:
            cam, sc = self.ms.camera, self.ms.scene
            self._guides[w, h] = self.dev.render_guides(cam, sc, w, h) + (self.dev.render_albedo(cam, sc, w, h),)
        return self._guides[w, h]

    def denoised(self, fmt, w=W, h=H, **kw):
        fb = self.render(fmt, w, h)
        self.dev.denoise(self.ms.camera, self.ms.scene, fb, **kw)
        return mapped(self.dev, fb, fmt, w, h)

    def expect(self, fmt, w=W, h=H, iterations=5, power=POWER):
        """The numpy demodulated filter on the GPU's own undenoised frame, guides and albedo."""
        px = pixels(self.raw(fmt, w, h), fmt, w)[..., :3]
        c0 = px.astype(np.float64) / 255.0 if px.dtype == np.uint8 else px.astype(np.float64)
        pos, nrm, alb = self.guides(w, h)
        return aref.demodulated_atrous(c0, pos, nrm, alb, iterations, power, FLOOR, **DEFAULTS)


@pytest.fixture(scope="module")
def plain(gpu_device):
    return Plain(gpu_device)


@pytest.fixture(scope="module")
def special(gpu_device):
    return Special(gpu_device)


@pytest.fixture(scope="module")
def textured(gpu_device):
    return Textured(gpu_device)


# ----------------------------------------------------------------------------- CPU
def _host_scene(host_device):
    (near, _, _), (tilt, _, _) = ref.two_quads()
    ms = aref.MaterialScene(host_device, [(near, _matte(host_device, MATTE_A)), (tilt, _matte(host_device, MATTE_B))])
    return ms, host_device.rtNewFrameBuffer("RGB_FLOAT32", 8, 8)


def test_host_device_refuses_albedo(host_device):
    ms, _ = _host_scene(host_device)
    with pytest.raises(RuntimeError, match="host-only"):
        host_device.render_albedo(ms.camera, ms.scene, 8, 8)


def test_denoise_params_grow_by_size(host_device):
    full = C.sizeof(N.DenoiseParams)
    assert full == OLD_SIZE + 12
    p = N.DenoiseParams(size=full, demodulate=-7, albedoPower=-7, albedoFloor=-7)
    assert N.dev.yrtDenoiseDefaults(C.byref(p)) == 0
    assert (p.demodulate, p.albedoPower, p.albedoFloor) == (0, 1.0, float(np.float32(1) / np.float32(255)))
    p = N.DenoiseParams(size=OLD_SIZE, demodulate=-7, albedoPower=-7, albedoFloor=-7)
    assert N.dev.yrtDenoiseDefaults(C.byref(p)) == 0
    assert (p.iterations, p.sigmaColor, p.sigmaNormal) == (5, 1.0, 64.0)
    assert (p.demodulate, p.albedoPower, p.albedoFloor) == (-7, -7, -7)
    # the new fields are validated only when demodulate is set
    ms, fb = _host_scene(host_device)
    base = dict(size=full, iterations=1, sigmaColor=1, sigmaNormal=64, sigmaPosition=0.02, albedoFloor=FLOOR)
    p = N.DenoiseParams(demodulate=1, albedoPower=0, **base)
    assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
    assert "albedoPower" in host_device.error() and "host-only" not in host_device.error()
    p = N.DenoiseParams(demodulate=0, albedoPower=0, **base)
    assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
    assert "host-only" in host_device.error()
    for bad in (dict(albedoPower=float("inf")), dict(albedoPower=float("nan")), dict(albedoPower=1, albedoFloor=0)):
        p = N.DenoiseParams(demodulate=1, **{**base, **bad})
        assert N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb, C.byref(p)) != 0
        assert "albedo" in host_device.error() and "host-only" not in host_device.error(), bad


def test_denoise_defaults_keys():
    assert yrt.Device.denoise_defaults() == dict(iterations=5, **DEFAULTS)
    assert yrt.Device.denoise_defaults(extended=True) == dict(iterations=5, demodulate=0, albedo_power=1.0,
                                                              albedo_floor=FLOOR, **DEFAULTS)


def test_denoise_albedo_tag_parses(host_device):
    yrt.Session(c1_args(16) + ["-denoise-albedo", "1"], device=host_device).close()
    yrt.Session(c1_args(16) + ["-denoise", "3", "-denoise-albedo", "1"], device=host_device).close()
    yrt.Session(c1_args(16) + ["-denoise-albedo", "0", "-denoise", "3"], device=host_device).close()
    with pytest.raises(RuntimeError, match="-denoise-albedo"):
        yrt.Session(c1_args(16) + ["-denoise-albedo", "2"], device=host_device)


# ----------------------------------------------------------------------------- GPU, albedo
@pytest.mark.gpu
def test_albedo_of_plain_materials(plain):
    """Matte: the albedo is the float32 reflectance of the quad hit, bit for bit; w = 1 on a hit and
    the whole pixel +0 on a miss, the hit mask being render_guides'."""
    pos, alb = plain.pos, plain.albedo
    hit = np.isfinite(pos[..., 3])
    near = hit & (np.abs(pos[..., 2] - ref.QUAD_NEAR_Z) < 1e-3)
    tilt = hit & ~near
    assert near.sum() > 50 and tilt.sum() > 50 and (~hit).sum() > 50
    assert np.array_equal(alb[near][:, :3], np.broadcast_to(np.float32(MATTE_A), (near.sum(), 3)))
    assert np.array_equal(alb[tilt][:, :3], np.broadcast_to(np.float32(MATTE_B), (tilt.sum(), 3)))
    assert np.all(alb[hit][:, 3] == 1)
    assert np.array_equal(alb[..., 3] != 0, hit)
    assert np.array_equal(alb[~hit].view(np.uint32), np.zeros(alb[~hit].shape, np.uint32))  # +0, not -0


@pytest.mark.gpu
def test_albedo_without_a_diffuse_component(special):
    """A Mirror has no diffuse component and a light primitive is no surface to demodulate: (1, 1, 1).
    The Obj quad's albedo is d Kd map_Kd in float32, bit for bit on the pixels whose (s, t), read off
    the hit point, lies farther than 1e-4 from a texel boundary."""
    d, ms = special.ms.dev, special.ms
    pos, _ = d.render_guides(ms.camera, ms.scene, W, H)
    alb = d.render_albedo(ms.camera, ms.scene, W, H)
    hit = np.isfinite(pos[..., 3])
    near = hit & (np.abs(pos[..., 2] - ref.QUAD_NEAR_Z) < 1e-3)
    light = hit & (np.abs(pos[..., 2] - LIGHT_Z) < 1e-3)
    mirror = hit & ~near & ~light
    assert near.sum() > 50 and mirror.sum() > 50 and light.sum() >= 10
    assert np.all(alb[mirror] == 1) and np.all(alb[light] == 1)
    assert np.array_equal(alb[..., 3] != 0, hit)
    # the near quad of denoise_ref.two_quads: x in [-1, 1/4], y in [-1/2, 1/2]
    s, t = (pos[near][:, 0].astype(np.float64) + 1) / 1.25, pos[near][:, 1].astype(np.float64) + 0.5
    far = aref.texel_boundary_distance(s, t, 4, 4) > 1e-4
    assert far.mean() >= 0.9
    want = (np.float32(1.0) * np.float32(OBJ_KD)) * aref.lookup_nearest(special.kd_image, s, t)
    assert want.dtype == np.float32
    assert np.array_equal(alb[near][far][:, :3], want[far])


@pytest.mark.gpu
def test_albedo_of_a_texture(textured):
    """MatteTextured: the albedo is the texture lookup at the hit's (s, t), reconstructed here from
    pos4 and the quads' parametrisation (aref.quad_st).
    nearest (8 x 8): bit-exact on the pixels farther than 1e-4 from a texel boundary (ST_ERR is 40
    times smaller).
    bilinear (4 x 4): the lookup is piecewise linear and continuous in (s, t) with slopes of at most
    one neighbour difference per texel, so the two sides differ by at most ST_ERR (W Dx + H Dy)
    (Dx = 3/256, Dy = 12/256, aref.texture_image: 5.9e-7) plus the float32 lookup's own rounding, 4 ulp
    of the largest texel (four products, three sums and the two ratios: 2.4e-7). Pixels within 1e-4 of
    the quad's border, where s1 = s - floor(s) wraps, are left out."""
    pos, _, alb = textured.guides()
    hit = np.isfinite(pos[..., 3])
    near = hit & (np.abs(pos[..., 2] - 2.0) < 1e-3)
    tilt = hit & ~near
    assert near.sum() > 50 and tilt.sum() > 50 and (~hit).sum() > 50
    assert np.all(alb[hit][:, 3] == 1)

    s, t = aref.quad_st(pos[near], near=True)
    far = aref.texel_boundary_distance(s, t, 8, 8) > 1e-4
    want = aref.lookup_nearest(textured.img_near, s, t)
    assert len(np.unique(want[far][:, 0])) > 20, "many texels in view"
    assert np.array_equal(alb[near][far][:, :3], want[far])

    s2, t2 = aref.quad_st(pos[tilt], near=False)
    inside = (np.minimum(s2, 1 - s2) > 1e-4) & (np.minimum(t2, 1 - t2) > 1e-4)
    img = textured.img_tilt
    tol = 4 * float(np.spacing(img.max())) + ST_ERR * (4 * 3 / 256 + 4 * 12 / 256)
    err = np.abs(alb[tilt][:, :3].astype(np.float64) - aref.lookup_bilinear(img, s2, t2))[inside]
    compared = (far.sum() + inside.sum()) / hit.sum()
    print(f"albedo of a texture: nearest {far.sum()} of {near.sum()} pixels exact, bilinear error {err.max():.3g} "
          f"(tolerance {tol:.3g}) on {inside.sum()} of {tilt.sum()}; compared {compared:.3f} of the hits")
    assert compared >= 0.9
    assert err.max() <= tol
    assert np.ptp(alb[tilt][:, 0]) > 0.1, "the texture varies over the quad"


@pytest.mark.gpu
def test_bump_map_does_not_reach_the_normal_guide(special):
    """Obj's bump map acts on a copy of the differential geometry: the normal guide is postIntersect's
    flat normal before and after an albedo pass (the map of `Special` would turn it round)."""
    d, ms = special.ms.dev, special.ms
    before = d.render_guides(ms.camera, ms.scene, W, H)
    d.render_albedo(ms.camera, ms.scene, W, H)
    after = d.render_guides(ms.camera, ms.scene, W, H)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pos, nrm = after
    near = np.isfinite(pos[..., 3]) & (np.abs(pos[..., 2] - ref.QUAD_NEAR_Z) < 1e-3)
    assert np.abs(nrm[near][:, :3] - ref.N_NEAR).max() <= 5 * 2.0 ** -23


# ----------------------------------------------------------------------------- GPU, filter
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_demodulated_filter_matches_numpy(textured, fmt, iterations):
    """|gpu - numpy| / max(|numpy|, 1/255) <= 1.4e-4 (DEMOD_BOUND) on the textured quads with
    albedo_power 1 / 2.2. Measured on an MI355X: 6.9e-7, 1.19e-6 and 1.02e-6 for 1, 3 and 5 iterations
    (either float format)."""
    raw = pixels(textured.raw(fmt), fmt, W)
    assert (raw[..., :3].max(-1) > 0.01).mean() > 0.2, "the scene must be lit"
    got = pixels(textured.denoised(fmt, iterations=iterations, demodulate=1, albedo_power=POWER), fmt, W)
    want = textured.expect(fmt, iterations=iterations)
    hit = np.isfinite(textured.guides()[0][..., 3])
    dev = reldev(got[..., :3][hit], want[hit])
    print(f"demodulated filter {fmt} x{iterations}: relative deviation {dev:.3g}")
    assert np.abs(got[..., :3][hit].astype(np.float64) - raw[..., :3][hit]).max() > 1e-3, "the filter must act"
    assert dev <= DEMOD_BOUND
    assert np.array_equal(got[~hit].view(np.uint32), raw[~hit].view(np.uint32))
    if fmt == "RGBA_FLOAT32":
        assert np.array_equal(got[..., 3], raw[..., 3])


@pytest.mark.gpu
def test_demodulated_filter_rgb8(textured):
    """Bytes within 1 of the numpy result quantized the same way; the padded bytes of the RGB8 rows
    (width 38: 114 of 116) and the miss pixels are untouched."""
    d, fmt = textured.dev, "RGB8"
    fb = textured.render(fmt, W8, H)
    raw = mapped(d, fb, fmt, W8, H)
    raw[:, 3 * W8:] = 0xA5  # mark the padding, so that a store into it shows
    mapped(d, fb, fmt, W8, H, write=raw)
    d.denoise(textured.ms.camera, textured.ms.scene, fb, demodulate=1, albedo_power=POWER)
    out = mapped(d, fb, fmt, W8, H)
    got, before = pixels(out, fmt, W8), pixels(raw, fmt, W8)
    assert np.array_equal(pixels(textured.raw(fmt, W8, H), fmt, W8), before)
    want = ref.quantize(textured.expect(fmt, W8, H))
    hit = np.isfinite(textured.guides(W8, H)[0][..., 3])
    diff = np.abs(got[hit].astype(int) - want[hit].astype(int))
    print(f"demodulated filter RGB8: {float((diff > 0).mean()):.4f} of the bytes differ by 1, max {diff.max()}")
    assert diff.max() <= 1
    assert (got[hit] != before[hit]).mean() > 0.2, "the filter must act"
    assert np.array_equal(got[~hit], before[~hit])
    assert np.all(out[:, 3 * W8:] == 0xA5)


@pytest.mark.gpu
def test_pure_texture_passes_through(textured):
    """A frame that is texture and nothing else, v m_p on the hit pixels with m from numpy's float32
    powf: the demodulated filter returns it within 8 ulp (one for the division, the constant-frame
    rule's two, one for the product, doubled for yrt_powf and numpy's powf disagreeing in the last
    place), while the plain filter without a colour weight blurs it by more than 1 %. Measured on an MI355X:
    2 ulp, and 43 % for the plain filter."""
    d, fmt = textured.dev, "RGB_FLOAT32"
    pos, _, alb = textured.guides()
    hit = np.isfinite(pos[..., 3])
    m = aref.modulation(alb, POWER, FLOOR, dtype=np.float32)
    assert m.dtype == np.float32
    value = np.float32([0.7231, 0.05, 3.5])
    frame = np.full((H, W, 3), np.float32(9.0))
    frame[hit] = value * m[hit]

    def filtered(**kw):
        fb = textured.render(fmt)
        mapped(d, fb, fmt, W, H, write=frame.view(np.uint8).reshape(H, -1))
        d.denoise(textured.ms.camera, textured.ms.scene, fb, **kw)
        return pixels(mapped(d, fb, fmt, W, H), fmt, W)

    out = filtered(demodulate=1, albedo_power=POWER)
    ulps = np.abs(out[hit] - frame[hit]) / np.spacing(frame[hit])
    plain = filtered(demodulate=0, sigma_color=0)
    blur = (np.abs(plain[hit] - frame[hit]) / frame[hit]).max()
    print(f"pure texture: demodulated within {ulps.max():.1f} ulp, the plain filter changes a pixel by {blur:.3f}")
    assert ulps.max() <= 8
    assert np.array_equal(out[~hit], frame[~hit])
    assert blur > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_demodulate_zero_is_the_plain_filter(textured, fmt):
    """demodulate = 0, the default, and the struct that ends before the field: byte-identical frames."""
    w = W8 if fmt == "RGB8" else W
    d, cam, sc = textured.dev, textured.ms.camera, textured.ms.scene
    default = pixels(textured.denoised(fmt, w, H), fmt, w)
    off = pixels(textured.denoised(fmt, w, H, demodulate=0, albedo_power=0.25, albedo_floor=0.5), fmt, w)
    fb = textured.render(fmt, w, H)
    p = N.DenoiseParams(size=OLD_SIZE, demodulate=1, albedoPower=-1, albedoFloor=-1)  # beyond size: not read
    assert N.dev.yrtDenoiseDefaults(C.byref(p)) == 0
    assert N.dev.yrtDenoiseFrameBuffer(d.h, cam, sc, fb, C.byref(p)) == 0, d.error()
    old = pixels(mapped(d, fb, fmt, w, H), fmt, w)
    assert not np.array_equal(default, pixels(textured.raw(fmt, w, H), fmt, w))
    assert np.array_equal(default.view(np.uint8), off.view(np.uint8))
    assert np.array_equal(default.view(np.uint8), old.view(np.uint8))
    on = pixels(textured.denoised(fmt, w, H, demodulate=1), fmt, w)
    assert not np.array_equal(default, on)


@pytest.mark.gpu
def test_cube_job_faces_demodulated(textured):
    """Two frames of one rtRenderFrames job (the second seen from the side), each denoised with
    demodulation through its own camera while both still lie in the job's frame block. Measured on an
    MI355X: 9.2e-7 and 1.14e-6."""
    from test_cpu_host import yrt_lookat
    d, ms, S = textured.dev, textured.ms, 32
    cam2 = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam2, "local2world", yrt_lookat((-1.5, 0.3, 0.5), (0.5, 0, 3.5), (0, 1, 0)))
    d.rtSetFloat1(cam2, "angle", 70.0)
    d.rtSetFloat1(cam2, "aspectRatio", 1.0)
    d.rtCommit(cam2)
    cams = [ms.camera, cam2]

    def job():
        fbs = [d.rtNewFrameBuffer("RGB_FLOAT32", S, S) for _ in cams]
        d.rtRenderFrames(textured.renderer, cams, ms.scene, textured.tm, fbs, 0)
        return fbs

    raws = [d.framebuffer_array(fb, S, S, "RGB_FLOAT32") for fb in job()]
    fbs = job()
    for fb, cam in zip(fbs, cams):
        d.denoise(cam, ms.scene, fb, iterations=3, demodulate=1, albedo_power=POWER)
    assert not np.array_equal(raws[0], raws[1])
    for fb, cam, raw in zip(fbs, cams, raws):
        got = d.framebuffer_array(fb, S, S, "RGB_FLOAT32")
        pos, nrm = d.render_guides(cam, ms.scene, S, S)
        alb = d.render_albedo(cam, ms.scene, S, S)
        hit = np.isfinite(pos[..., 3])
        assert 50 < hit.sum() < S * S
        want = aref.demodulated_atrous(raw, pos, nrm, alb, 3, POWER, FLOOR, **DEFAULTS)
        dev = reldev(got[hit], want[hit])
        print(f"cube face, demodulated: relative deviation {dev:.3g}")
        assert dev <= DEMOD_BOUND
        assert np.array_equal(got[~hit], raw[~hit]) and not np.array_equal(got[hit], raw[hit])


# ----------------------------------------------------------------------------- GPU, it denoises
@pytest.mark.gpu
def test_demodulation_denoises_textured_frames_better(gpu_device, tmp_path):
    """The textured room (aref.write_room: the Cornell box with MatteTextured walls and a block, depth
    5) at 64 x 64, gamma 2.2: the 4-spp frame filtered with demodulation (albedo_power 1 / 2.2, otherwise
    the defaults) is closer to the 1024-spp frame than both the raw frame and the default filter's, in
    mean squared error over the pixels below 1 in both frames. CPU rehearsal
    (tools/denoise_albedo_rehearsal.py: the oracle's frames, the numpy filter and a numpy albedo):
    demodulated / raw 0.337, demodulated / plain 0.418; on an MI355X the same 0.3371 and 0.4183, the
    frames being the oracle's (which also has the Sponza stand-in, whose textures a
    64 x 64 frame cannot resolve).
    And the front end's `-denoise 5 -denoise-albedo 1 -gamma 2.2` is that frame bit for bit."""
    S = 64
    d = gpu_device
    xml = aref.write_room(tmp_path)
    s = yrt.Session(aref.room_args(xml, S, 1024), device=d)
    conv = s.render().astype(np.float64)
    s.close()
    s = yrt.Session(aref.room_args(xml, S, 4), device=d)
    raw = s.render().astype(np.float64)
    i = s.info()

    def filtered(**kw):
        s.render(read=False)
        d.denoise(s.camera(), i["scene"], i["framebuffer"], **kw)
        return d.framebuffer_array(i["framebuffer"], S, S, "RGB_FLOAT32").astype(np.float64)

    plain = filtered()
    demod = filtered(demodulate=1, albedo_power=POWER)
    s.close()
    assert "-gamma" in aref.room_args(xml, S, 4) and "2.2" in aref.room_args(xml, S, 4)
    s = yrt.Session(aref.room_args(xml, S, 4) + ["-denoise", "5", "-denoise-albedo", "1"], device=d)
    tagged = s.render().astype(np.float64)
    s.close()
    dark = (conv.max(-1) < 1) & (raw.max(-1) < 1)
    assert dark.mean() > 0.9
    mse_raw, mse_plain, mse_demod = (((f - conv)[dark] ** 2).mean() for f in (raw, plain, demod))
    print(f"room 64x64 gamma 2.2, pixels below 1 ({dark.mean():.3f} of the frame): mse raw {mse_raw:.6g} plain "
          f"{mse_plain:.6g} demodulated {mse_demod:.6g}; demodulated / raw {mse_demod / mse_raw:.4f}, "
          f"demodulated / plain {mse_demod / mse_plain:.4f}")
    assert mse_demod < mse_plain
    assert mse_demod < mse_raw
    assert np.array_equal(tagged, demod), "-denoise 5 -denoise-albedo 1 is the demodulated default filter"
