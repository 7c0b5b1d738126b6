"""The variance-guided denoiser on the device ("variance-guided"): the variance frame
(yrtFrameVariance, k_frame_variance) against the shared header on the host bit for bit and against
float64, the variance-guided filter (k_atrous_load_var, k_atrous_var) against the float64 numpy
restatement of tests/denoise_variance_ref.py on the GPU's own frames, guides and variance frames,
for a frame, a demodulated frame and a cube; the refusals; and whether it denoises."""
from __future__ import annotations

import numpy as np
import pytest

import yrt

import denoise_cube_ref as cref
import denoise_ref as ref
import denoise_variance_ref as vref
from adaptive_ref import sums_after
from denoise_albedo_ref import mapped, modulation, pixels, reldev
from helpers import c1_args
from test_adaptive import CASES, Adaptive
from trace_scenes import MeshScene

pytestmark = pytest.mark.gpu

W, H = 40, 24          # not a multiple of the 16-pixel tile
FORMATS = ("RGB8", "RGBA8", "RGB_FLOAT32", "RGBA_FLOAT32")
WEIGHTS = dict(sigma_normal=64.0, sigma_position=float(np.float32(0.02)))
DEFAULTS = yrt.Device.denoise_defaults(variance=True)
SV, FLOOR = DEFAULTS["sigma_variance"], DEFAULTS["variance_floor"]

# Largest |gpu - float64| / max(float64, varianceFloor) of the variance frame measured on an MI355X
# over test_variance_frame_against_float64's cases (gamma 2.2 without and with the vignette); the
# bound is 8 x that, under the hard ceiling 1e-4. DESIGN.md §9 records both. Measured: 1.82e-5 and
# 2.62e-5 (the host's header gives the same two figures), where two displayed halves near 1 differ
# by a few thousandths and powf's last bits do not cancel; 8 x 2.62e-5 exceeds the ceiling, which
# therefore is the bound.
VARIANCE_MEASURED = 2.62e-5
VARIANCE_BOUND = min(8 * VARIANCE_MEASURED, 1e-4)
# Largest |gpu - numpy| / max(|numpy|, 1/255) of the variance-guided filter measured on an MI355X over
# the float cases below (frame 1, 3, 5 iterations, demodulated, cube inside and across the edges);
# the bound is 8 x that, under the plain filter's ceiling 1e-4 (tests/test_denoise.py). Measured:
# 5.12e-7, 6.36e-7 and 6.36e-7 for 1, 3 and 5 iterations (either float format), 6.73e-7 demodulated,
# 1.41e-6 inside the cube's faces and 3.30e-6 across its edges (the box's coordinates are in the
# hundreds). RGB8 and RGBA8: every byte equal to the quantized numpy result.
FILTER_MEASURED = 3.30e-6
FILTER_BOUND = min(8 * FILTER_MEASURED, 1e-4)


class Quads:
    """tests/test_denoise.py's two-quad scene under its emissive triangle, a 4-spp depth-2 path
    tracer and a default tone mapper with the given gamma and vignette. Frames are adaptive renders
    with threshold 0: `iterations` plain progressive frames."""

    def __init__(self, dev, gamma=1.0, vignetting=False):
        self.dev = dev
        self.ms = MeshScene(dev, ref.two_quads(), eye=(0, 0, 0), look=(0, 0, 1), up=(0, 1, 0), angle=60.0)
        ref.add_triangle_light(self.ms)
        self.renderer = dev.rtNewRenderer("pathtracer")
        dev.rtSetInt1(self.renderer, "maxDepth", 2)
        dev.rtSetInt1(self.renderer, "sampler.spp", 4)
        dev.rtCommit(self.renderer)
        self.tm = dev.rtNewToneMapper("default")
        dev.rtSetFloat1(self.tm, "gamma", gamma)
        dev.rtSetBool1(self.tm, "vignetting", vignetting)
        dev.rtCommit(self.tm)
        self._guides = self._albedo = None
        self._raw = {}

    def adaptive(self, fmt, iterations=2, fb=None):
        """A framebuffer holding the frame, not mapped yet."""
        fb = fb or self.dev.rtNewFrameBuffer(fmt, W, H)
        self.dev.rtRenderAdaptive(self.renderer, self.ms.camera, self.ms.scene, self.tm, fb, threshold=0.0,
                                  max_iterations=iterations)
        return fb

    def plain(self, fmt, fb=None):
        fb = fb or self.dev.rtNewFrameBuffer(fmt, W, H)
        self.dev.rtRenderFrame(self.renderer, self.ms.camera, self.ms.scene, self.tm, fb, 0)
        return fb

    def raw(self, fmt):
        """The undenoised adaptive frame's mapped bytes. Shared: do not modify."""
        if fmt not in self._raw:
            self._raw[fmt] = mapped(self.dev, self.adaptive(fmt), fmt, W, H)
            self._raw[fmt].setflags(write=False)
        return self._raw[fmt]

    def guides(self):
        if self._guides is None:
            self._guides = self.dev.render_guides(self.ms.camera, self.ms.scene, W, H)
        return self._guides

    def hit(self):
        return np.isfinite(self.guides()[0][..., 3])

    def albedo(self):
        if self._albedo is None:
            self._albedo = self.dev.render_albedo(self.ms.camera, self.ms.scene, W, H)
        return self._albedo

    def denoise(self, fb, **kw):
        self.dev.denoise(self.ms.camera, self.ms.scene, fb, **kw)

    def sums(self, iterations=2):
        """The oracle's sums and half sums of the frame: the device's, bit for bit (test_adaptive.py)."""
        blob = self.dev.export_frame(self.renderer, self.ms.camera, self.ms.scene)
        return sums_after(blob, W, H, iterations)


@pytest.fixture(scope="module")
def quads(gpu_device):
    return Quads(gpu_device)


def _c0(px):
    px = px[..., :3]
    return px.astype(np.float64) / 255.0 if px.dtype == np.uint8 else px.astype(np.float64)


# ----------------------------------------------------------------------------- a, b: the variance frame
def test_variance_frame_is_the_header_tile_by_tile(gpu_device):
    """test_adaptive.py's "partial" case (Cornell box 40 x 24, 4 spp, threshold 0.13, 8 iterations):
    tiles stop at different counts, some are partial. Every tile of yrtFrameVariance equals
    yrt.frame_variance (the header on the host) of the oracle's sums after that tile's own count."""
    args, thr, cap = CASES["partial"]
    p = Adaptive(gpu_device, args())
    try:
        assert p.gamma == 1.0
        _, st, it, _ = p.adaptive(thr, cap)
        var = gpu_device.frame_variance(p.i["framebuffer"])
        assert var.shape == (p.H, p.W, 4) and var.dtype == np.float32
        assert len(set(it.tolist())) >= 2 and (p.W % 16 or p.H % 16)
        tx = (p.W + 15) // 16
        for t, n in enumerate(it.tolist()):
            ys, xs = slice(16 * (t // tx), 16 * (t // tx) + 16), slice(16 * (t % tx), 16 * (t % tx) + 16)
            want = yrt.frame_variance(*sums_after(p.blob, p.W, p.H, n))[ys, xs]
            assert np.array_equal(var[ys, xs].view(np.uint32), want.view(np.uint32)), (t, n)
        assert (var[..., :3] > 0).mean() > 0.5 and (var[..., 3] == 1).all()
    finally:
        p.close()


@pytest.mark.parametrize("vignetting", [False, True])
def test_variance_frame_against_float64(gpu_device, vignetting):
    """Gamma 2.2, without and with the vignette, on the two-quad scene: |gpu - float64| /
    max(float64, varianceFloor) within VARIANCE_BOUND. Measured on an MI355X: see VARIANCE_MEASURED.
    The same render with gamma 1 first shows that the oracle's sums are the device's."""
    lin = Quads(gpu_device)
    accu, half = lin.sums()
    got = gpu_device.frame_variance(lin.adaptive("RGB_FLOAT32"))
    assert np.array_equal(got.view(np.uint32), yrt.frame_variance(accu, half).view(np.uint32))
    q = Quads(gpu_device, 2.2, vignetting)
    got = gpu_device.frame_variance(q.adaptive("RGB_FLOAT32")).astype(np.float64)
    want = vref.frame_variance_f64(accu, half, 2.2, vignetting)
    assert (want[..., :3] > FLOOR).mean() > 0.1, "the scene must be noisy"
    err = float((np.abs(got[..., :3] - want[..., :3]) / np.maximum(want[..., :3], FLOOR)).max())
    print(f"variance frame, gamma 2.2, vignette {vignetting}: |gpu - float64| / max(float64, floor) {err:.3g}")
    assert np.array_equal(got[..., 3], want[..., 3])
    assert err <= VARIANCE_BOUND


# ----------------------------------------------------------------------------- c: the filter
def _expect(q, fmt, iterations, var4, m=None):
    c0 = _c0(pixels(q.raw(fmt), fmt, W))
    pos, nrm = q.guides()
    return vref.atrous_var(c0, var4, pos, nrm, iterations, SV, FLOOR, m=m, **WEIGHTS)


@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_matches_numpy(quads, fmt, iterations):
    """Measured on an MI355X: see FILTER_MEASURED. Step 16 of the fifth iteration sends taps outside
    the 40 x 24 frame on every side."""
    fb = quads.adaptive(fmt)
    var4 = quads.dev.frame_variance(fb)
    quads.denoise(fb, iterations=iterations, variance_guided=1)
    got = pixels(mapped(quads.dev, fb, fmt, W, H), fmt, W)
    raw = pixels(quads.raw(fmt), fmt, W)
    want = _expect(quads, fmt, iterations, var4)
    hit = quads.hit()
    assert (raw[..., :3].max(-1) > 0.01).mean() > 0.2, "the scene must be lit"
    dev = reldev(got[..., :3][hit], want[hit])
    print(f"variance-guided filter {fmt} x{iterations}: relative deviation {dev:.3g}")
    assert np.abs(got[..., :3][hit].astype(np.float64) - raw[..., :3][hit]).max() > 1e-3, "the filter must act"
    assert dev <= FILTER_BOUND
    assert np.array_equal(got[~hit].view(np.uint32), raw[~hit].view(np.uint32))
    if fmt == "RGBA_FLOAT32":
        assert np.array_equal(got[..., 3], raw[..., 3])
    if iterations == 5:  # and it is another filter than the plain one
        plain = ref.atrous(_c0(raw), *quads.guides(), 5, sigma_color=1.0, **WEIGHTS)
        assert reldev(got[..., :3][hit], plain[hit]) > 100 * FILTER_BOUND


@pytest.mark.parametrize("fmt", ["RGB8", "RGBA8"])
def test_filter_8bit(quads, fmt):
    """Bytes within 1 of the numpy result quantized the same way; alpha and misses untouched."""
    fb = quads.adaptive(fmt)
    var4 = quads.dev.frame_variance(fb)
    quads.denoise(fb, variance_guided=1)
    got = pixels(mapped(quads.dev, fb, fmt, W, H), fmt, W)
    before = pixels(quads.raw(fmt), fmt, W)
    want = ref.quantize(_expect(quads, fmt, 5, var4))
    hit = quads.hit()
    diff = np.abs(got[..., :3][hit].astype(int) - want[hit].astype(int))
    print(f"variance-guided filter {fmt}: {float((diff > 0).mean()):.4f} of the bytes differ by 1, max {diff.max()}")
    assert diff.max() <= 1
    assert (got[..., :3][hit] != before[..., :3][hit]).mean() > 0.2, "the filter must act"
    assert np.array_equal(got[~hit], before[~hit])
    if fmt == "RGBA8":
        assert np.array_equal(got[..., 3], before[..., 3])


def test_demodulated_filter_matches_numpy(quads):
    fmt = "RGB_FLOAT32"
    fb = quads.adaptive(fmt)
    var4 = quads.dev.frame_variance(fb)
    quads.denoise(fb, variance_guided=1, demodulate=1, albedo_power=1.0)
    got = pixels(mapped(quads.dev, fb, fmt, W, H), fmt, W)
    d = yrt.Device.denoise_defaults(extended=True)
    m = modulation(quads.albedo(), 1.0, d["albedo_floor"])
    hit = quads.hit()
    assert (m[hit] != 1).all(), "the quads' albedo must act"
    want = _expect(quads, fmt, 5, var4, m=m)
    dev = reldev(got[hit], want[hit])
    print(f"variance-guided demodulated filter: relative deviation {dev:.3g}")
    assert dev <= FILTER_BOUND
    # one albedo everywhere scales the signal by 1 / m and its variance by 1 / m^2: only the floor's
    # share of the weight changes (2.2e-4 of the pixel, measured), still far outside the bound
    assert reldev(got[hit], _expect(quads, fmt, 5, var4)[hit]) > 2 * FILTER_BOUND, "the modulation must act"


# ----------------------------------------------------------------------------- d: off is off
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGB8"])
def test_mode_off_is_the_plain_filter(quads, fmt):
    """variance_guided = 0 through the long struct, with fields the mode would refuse: the default
    call byte for byte, on a plain frame and on an adaptive one."""
    for render in (quads.plain, quads.adaptive):
        a, b = render(fmt), render(fmt)
        quads.denoise(a)
        quads.denoise(b, variance_guided=0, sigma_variance=-1.0, variance_floor=float("nan"))
        assert np.array_equal(mapped(quads.dev, a, fmt, W, H), mapped(quads.dev, b, fmt, W, H))


# ----------------------------------------------------------------------------- e: refusals
def test_refusals_leave_the_frame(quads):
    d, fmt = quads.dev, "RGB_FLOAT32"

    def refused(fb, match, reference):
        with pytest.raises(RuntimeError, match=match):
            quads.denoise(fb, variance_guided=1)
        with pytest.raises(RuntimeError, match=match):
            d.frame_variance(fb)
        assert np.array_equal(mapped(d, fb, fmt, W, H), reference)

    plain = mapped(d, quads.plain(fmt), fmt, W, H)
    refused(quads.plain(fmt), "not an adaptive render", plain)
    one = quads.adaptive(fmt, iterations=1)
    assert (d.adaptive_tiles(one)[0] == 1).all()
    refused(one, "fewer than 2 iterations", plain)  # one iteration is the plain frame
    after = quads.plain(fmt, fb=quads.adaptive(fmt))
    refused(after, "not an adaptive render", plain)
    # and the parameters, judged before the frame is
    fb = quads.adaptive(fmt)
    for kw in (dict(sigma_variance=0.0), dict(variance_floor=float("inf"))):
        with pytest.raises(RuntimeError, match="varianceGuided"):
            quads.denoise(fb, variance_guided=1, **kw)
    assert np.array_equal(mapped(d, fb, fmt, W, H), quads.raw(fmt))
    quads.denoise(fb, variance_guided=1)  # the framebuffer still holds its adaptive render
    assert not np.array_equal(mapped(d, fb, fmt, W, H), quads.raw(fmt))


# ----------------------------------------------------------------------------- f: where it lives
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_is_filtered_where_it_lives(quads, fmt):
    d = quads.dev
    first = quads.adaptive(fmt)
    quads.denoise(first, variance_guided=1)
    first = mapped(d, first, fmt, W, H)
    fb = quads.adaptive(fmt)
    raw = mapped(d, fb, fmt, W, H)  # the frame now lives in the host pixels
    quads.denoise(fb, variance_guided=1)
    second = mapped(d, fb, fmt, W, H)
    assert not np.array_equal(second, raw)
    assert np.array_equal(pixels(first, fmt, W), pixels(second, fmt, W))


# ----------------------------------------------------------------------------- g: the cube
def test_cube_filter_matches_numpy(gpu_device):
    """One eye, six 24 x 24 faces, each rendered adaptively into its own framebuffer (threshold 0, 2
    iterations of 2 spp), 3 filter iterations: the pixels whose taps or 3x3 variance neighbours cross
    an edge and the others, each against the numpy cube filter."""
    d, S, fmt, its = gpu_device, 24, "RGB_FLOAT32", 3
    s = yrt.Session(cref.cube_args(S, 2), device=d)
    try:
        i = s.info()
        cams = [s.camera(f) for f in range(6)]
        fbs = [d.rtNewFrameBuffer(fmt, S, S) for _ in cams]
        for cam, fb in zip(cams, fbs):
            d.rtRenderAdaptive(i["renderer"], cam, i["scene"], i["tonemapper"], fb, threshold=0.0, max_iterations=2)
        raw = np.stack([d.framebuffer_array(fb, S, S, fmt) for fb in fbs])
        var4 = np.stack([d.frame_variance(fb) for fb in fbs])
        g = [d.render_guides(c, i["scene"], S, S) for c in cams]
        pos, nrm = np.stack([a for a, _ in g]), np.stack([b for _, b in g])
        d.denoise_cube(cams, i["scene"], fbs, iterations=its, variance_guided=1)
        got = np.stack([d.framebuffer_array(fb, S, S, fmt) for fb in fbs])
        with pytest.raises(RuntimeError, match="not an adaptive render"):
            job = [d.rtNewFrameBuffer(fmt, S, S) for _ in cams]
            d.rtRenderFrames(i["renderer"], cams, i["scene"], i["tonemapper"], job, 0)
            d.denoise_cube(cams, i["scene"], job, iterations=its, variance_guided=1)
    finally:
        s.close()
    want = vref.atrous_var_cube(raw, var4, pos, nrm, its, SV, FLOOR, **WEIGHTS)
    hit = np.isfinite(pos[..., 3])
    edge = np.broadcast_to(vref.crosses_edge(S, its), hit.shape)
    assert (hit & edge).sum() > 500 and (hit & ~edge).sum() > 100
    for name, sel in (("across the edges", hit & edge), ("inside", hit & ~edge)):
        dev = reldev(got[sel], want[sel])
        print(f"variance-guided cube filter, {name}: {int(sel.sum())} pixels, relative deviation {dev:.3g}")
        assert dev <= FILTER_BOUND
    assert np.array_equal(got[~hit], raw[~hit])
    # the edges matter: the per-face filter gives other pixels there
    faces = np.stack([vref.atrous_var(raw[f], var4[f], pos[f], nrm[f], its, SV, FLOOR, **WEIGHTS) for f in range(6)])
    assert reldev(got[hit & edge], faces[hit & edge]) > 100 * FILTER_BOUND


# ----------------------------------------------------------------------------- h, i: it denoises
def test_default_beats_the_plain_filter_on_c1(gpu_device):
    """C1 64 x 64, 2 iterations of 4 spp against the 1024-spp frame: the default variance-guided
    frame has a lower whole-frame error than the raw frame and than the plain default filter, and a
    lower below-1 error than the plain filter (CPU rehearsal, tools/denoise_variance_rehearsal.py:
    whole frame 0.671 against 1 and 0.988, below 1 0.220 against 0.355: more than 10 % each). And the
    front end's `-adaptive 0 2 -denoise 5 -denoise-variance 1` is that frame byte for byte."""
    S, d = 64, gpu_device
    s = yrt.Session(c1_args(S, 1024) + ["-fb", "RGB_FLOAT32"], device=d)
    conv = s.render().astype(np.float64)
    s.close()
    s = yrt.Session(c1_args(S, 4) + ["-fb", "RGB_FLOAT32"], device=d)
    i = s.info()

    def frame(**kw):
        d.rtRenderAdaptive(i["renderer"], s.camera(), i["scene"], i["tonemapper"], i["framebuffer"], threshold=0.0,
                           max_iterations=2)
        if kw:
            d.denoise(s.camera(), i["scene"], i["framebuffer"], **kw)
        return d.framebuffer_array(i["framebuffer"], S, S, "RGB_FLOAT32")

    raw, plain, guided = frame(), frame(iterations=5), frame(variance_guided=1)
    s.close()
    s = yrt.Session(c1_args(S, 4) + ["-fb", "RGB_FLOAT32", "-adaptive", "0", "2", "-denoise", "5", "-denoise-variance", "1"],
                    device=d)
    tagged = s.render()
    s.close()
    pw, pb = vref.mse_ratios(plain, raw, conv)
    gw, gb = vref.mse_ratios(guided, raw, conv)
    print(f"C1 64x64, 2 x 4 spp: plain whole {pw:.4f} below-1 {pb:.4f}; variance-guided whole {gw:.4f} below-1 {gb:.4f}")
    assert gw < 1.0 and gw < pw and gb < pb
    assert np.array_equal(tagged.view(np.uint32), guided.view(np.uint32))
