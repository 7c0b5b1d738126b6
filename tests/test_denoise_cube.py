"""The cube denoise ("cube"): yrtDenoiseCube filters the faces of a stereo cube as one
surface, a tap that leaves a face landing on the neighbouring face by the integer rule of
csrc/common/yrt_cube_tap.h. CPU: the rule against the table and against the cameras' geometry,
the refusals, the -denoise-cube tag. GPU: against the float64 numpy restatement of
tests/denoise_cube_ref.py, against the per-face filter, and whether the seam goes away."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import yrt
from yrt import _native as N

import denoise_cube_ref as cref
import denoise_ref as ref
from denoise_albedo_ref import mapped, pixels, reldev

W = 48                 # smaller than 2 * 2^4: at 5 iterations taps go deeper than half a face
W8 = 38                # 3 * 38 = 114 bytes per RGB8 row, padded to 116
DEFAULTS = dict(sigma_color=1.0, sigma_normal=64.0, sigma_position=float(np.float32(0.02)))  # the library's floats
POWER, FLOOR = 1 / 2.2, float(np.float32(1 / 255))
# test_denoise.py's derived ceilings: float32 epsilon x 25 taps x 5 iterations x the exponent 64 of
# the normal weight; demodulated: plus twice yrt_powf's 2e-5. The cube filter has the same tap
# count and the same weights. Measured on an MI355X over the cases below: 2.71e-6, 4.15e-6 and
# 6.92e-6 for 1, 3 and 5 iterations (RGB and RGBA float alike), 2.55e-6 demodulated at 5; RGB8 at
# width 38: no byte differs from the quantized numpy result.
FILTER_BOUND, DEMOD_BOUND = 1e-4, 1.4e-4


# ----------------------------------------------------------------------------- CPU: the tap rule
@pytest.fixture(scope="module")
def face_maps(host_device):
    """L_f (float64, 3 x 3, unit Frobenius norm) of the 12 faces of a -stereo session, fitted to
    oracle.camera_rays at the pixel centres: dir is proportional to L_f (px, 1 - py, 1)."""
    import oracle
    S = 48
    s = yrt.Session(cref.cube_args(S, 1), device=host_device)
    c = (np.arange(S, dtype=np.float32) + np.float32(0.5)) / np.float32(S)
    px = np.stack(np.meshgrid(c, c), -1).reshape(-1, 2)
    maps = []
    for f in range(12):
        _, dr = oracle.camera_rays(s.export_frame(f), px)
        Lf, residual = cref.face_linear_maps(dr, S)
        assert residual < 3e-7, (f, residual)
        maps.append(Lf)
    s.close()
    return maps


@pytest.mark.parametrize("width", [5, 16, 48])
def test_tap_rule_follows_the_table(width):
    """Every face, every tap with -64 <= qx, qy < W + 64: corner taps are skipped, in-face taps stay,
    crossing taps land inside the table's face; the library and the numpy restatement agree; and
    stepping back from where a tap lands leads to the face it came from, through the edge the
    symmetric table names."""
    crossing = 0
    for f in range(6):
        for qy in range(-64, width + 64):
            for qx in range(-64, width + 64):
                got = yrt.cube_tap(width, f, qx, qy)
                assert got == cref.cube_tap(width, f, qx, qy), (f, qx, qy)
                out_x, out_y = not 0 <= qx < width, not 0 <= qy < width
                if out_x and out_y:
                    assert got is None
                elif not out_x and not out_y:
                    assert got == (f, qx, qy)
                else:
                    e = (cref.L if qx < 0 else cref.R) if out_x else (cref.T if qy < 0 else cref.B)
                    g, e2, _ = cref.TABLE[f][e]
                    assert got[0] == g and 0 <= got[1] < width and 0 <= got[2] < width, (f, qx, qy, got)
                    crossing += 1
                    # the landing pixel lies in the half of g next to e2, and a tap from it straight
                    # out through e2 comes back to f through e
                    x2, y2 = got[1], got[2]
                    depth = {cref.L: x2, cref.R: width - 1 - x2, cref.T: y2, cref.B: width - 1 - y2}[e2]
                    assert 2 * depth < width
                    back = {cref.L: (-1, y2), cref.R: (width, y2), cref.T: (x2, -1), cref.B: (x2, width)}[e2]
                    home = yrt.cube_tap(width, g, *back)
                    assert home[0] == f and cref.TABLE[g][e2][:2] == (f, e), (f, e, g, e2, home)
    assert crossing == 6 * 4 * 64 * width
    for f in range(6):  # the table is symmetric: every pair from both sides, with one orientation
        for e in range(4):
            g, e2, rev = cref.TABLE[f][e]
            assert cref.TABLE[g][e2] == (f, e, rev)


def test_tap_rule_rejects_bad_arguments():
    g, x, y = C.c_int32(), C.c_int32(), C.c_int32()
    out = (C.byref(g), C.byref(x), C.byref(y))
    assert N.dev.yrtDebugCubeTap(48, 0, 3, 4, *out) == 1 and (g.value, x.value, y.value) == (0, 3, 4)
    assert N.dev.yrtDebugCubeTap(48, 0, -1, -1, *out) == 0
    for bad in ((0, 0, 0, 0), (16385, 0, 0, 0), (48, -1, 0, 0), (48, 6, 0, 0), (48, 0, 1 << 20, 0), (48, 0, 0, -(1 << 20))):
        assert N.dev.yrtDebugCubeTap(*bad, *out) == -1, bad
    assert N.dev.yrtDebugCubeTap(48, 0, 3, 4, None, None, None) == -1
    # the widest face and the deepest tap: the 32-bit products hold (against Python's integers)
    for q in ((16384 + (1 << 17) - 1, 16383), (-(1 << 17), 0), (5, 16384 + 70000), (16383, -70001)):
        assert yrt.cube_tap(16384, 3, *q) == cref.cube_tap(16384, 3, *q), q


@pytest.mark.parametrize("width", [5, 16, 48])
def test_tap_rule_matches_the_cameras(face_maps, width):
    """Against geometry, both eyes: the pixel a crossing tap returns is the one that contains the
    tap's direction L_f ((qx + .5) / W, 1 - (qy + .5) / W, 1) projected onto face g.

    The fitted maps carry the float32 rounding of the cameras' rotations (they agree with an ideal
    cube to about 3e-7, printed below), which moves a projected point by up to 1e-5 pixel at these
    widths; that decides nothing except at the exact ties that the rule's floor resolves (W = 48,
    k = 1, j = 15: the direction falls on the line between two pixels). So the check runs twice:
      - with the fitted maps as they are, for every tap whose projection lies farther than 1e-4
        pixel from a pixel border (the agreement the rule was derived to): it must lie in the
        returned pixel;
      - with the relative maps L_g^-1 L_f snapped to the nearest matrix of half-integers (an ideal
        cube's are exactly that; the snap must move no entry by more than 1e-5), for every tap,
        with a slack of 1e-6 pixel for the ties."""
    worst_snap = worst_slack = 0.0
    checked = ties = 0
    for eye in range(2):
        for f in range(6):
            Lf = face_maps[6 * eye + f]
            for e in range(4):
                g = cref.TABLE[f][e][0]
                G = np.linalg.solve(face_maps[6 * eye + g], Lf)
                G /= np.cbrt(np.linalg.det(G))  # the fitted maps have no scale; a rotation's relative map has det 1
                Gs = np.round(2 * G) / 2
                worst_snap = max(worst_snap, float(np.abs(G - Gs).max()))
                for k in range(64):
                    for j in range(width):
                        qx, qy = {cref.L: (-1 - k, j), cref.R: (width + k, j), cref.T: (j, -1 - k),
                                  cref.B: (j, width + k)}[e]
                        got = yrt.cube_tap(width, f, qx, qy)
                        assert got[0] == g
                        v = np.array([(qx + 0.5) / width, 1 - (qy + 0.5) / width, 1.0])
                        for M, every in ((G, False), (Gs, True)):
                            u = M @ v
                            assert u[2] > 0
                            x, y = u[0] / u[2] * width, (1 - u[1] / u[2]) * width
                            edge = min(abs(x - round(x)), abs(y - round(y)))
                            if not every and edge <= 1e-4:
                                ties += 1
                                continue
                            slack = max(got[1] - x, x - (got[1] + 1), got[2] - y, y - (got[2] + 1))
                            worst_slack = max(worst_slack, slack) if every else worst_slack
                            assert slack <= (1e-6 if every else 0.0), (eye, f, e, k, j, got, x, y)
                            checked += 1
    print(f"W {width}: {checked} projections, {ties} within 1e-4 pixel of a border left to the snapped maps; "
          f"snap moves an entry by at most {worst_snap:.3g}; worst slack with the snapped maps {worst_slack:.3g}")
    assert worst_snap <= 1e-5


# ----------------------------------------------------------------------------- CPU: refusals
@pytest.fixture(scope="module")
def host_cube(host_device):
    s = yrt.Session(cref.cube_args(16, 1), device=host_device)
    cams = [s.camera(f) for f in range(12)]
    fbs = [host_device.rtNewFrameBuffer("RGB_FLOAT32", 16, 16) for _ in range(12)]
    yield host_device, s, cams, fbs
    s.close()


def test_host_device_refuses_the_cube(host_cube):
    """A valid job passes the validation, which needs no GPU, and meets the other denoise calls'
    refusal."""
    d, s, cams, fbs = host_cube
    scene = s.info()["scene"]
    for sel in (slice(0, 12), slice(0, 6), slice(6, 12)):
        with pytest.raises(RuntimeError, match=r'host-only device \(created with parms "host"\)'):
            d.denoise_cube(cams[sel], scene, fbs[sel])
    order = [7, 3, 0, 11, 5, 2, 9, 1, 6, 10, 4, 8]  # any order
    with pytest.raises(RuntimeError, match="host-only"):
        d.denoise_cube([cams[k] for k in order], scene, fbs)


def test_cube_arguments_are_validated(host_cube):
    d, s, cams, fbs = host_cube
    scene = s.info()["scene"]

    def refused(cameras, framebuffers, match, **kw):
        with pytest.raises(RuntimeError, match=match) as e:
            d.denoise_cube(cameras, scene, framebuffers, **kw)
        assert "host-only" not in str(e.value)

    refused(cams[:5], fbs[:5], "6 .*or 12")
    refused(cams[:7], fbs[:7], "6 .*or 12")
    refused([], [], "6 .*or 12")
    pin = d.rtNewCamera("pinhole")
    d.rtCommit(pin)
    refused([pin] + cams[1:6], fbs[:6], "stereo")
    fresh = d.rtNewCamera("stereo")  # never committed
    refused([fresh] + cams[1:6], fbs[:6], "committed")
    refused(cams[:5] + [cams[0]], fbs[:6], "twice")
    refused(cams[:11] + [cams[3]], fbs, "twice")
    refused(cams[:5] + [cams[11]], fbs[:6], "one eye")
    refused(cams[:6], fbs[:5] + [d.rtNewFrameBuffer("RGB_FLOAT32", 16, 8)], "square")
    refused(cams[:6], fbs[:5] + [d.rtNewFrameBuffer("RGB_FLOAT32", 8, 8)], "one size")
    refused(cams[:6], fbs[:5] + [d.rtNewFrameBuffer("RGBA_FLOAT32", 16, 16)], "one format")
    refused(cams[:6], fbs[:5] + [fbs[0]], "twice")
    refused(cams[:6], fbs[:6], "iterations", iterations=17)  # p is read as yrtDenoiseFrameBuffer reads it
    # differing camera parameters: face 2 of another rig
    s2 = yrt.Session(cref.cube_args(16, 1) + ["-vp", "278", "273", "251"], device=d)
    refused(cams[:2] + [s2.camera(2)] + cams[3:6], fbs[:6], "differ")
    s2.close()
    # null handles and a short struct
    p = N.DenoiseParams(size=2, iterations=1)
    arr = (C.c_void_p * 6)(*cams[:6])
    fba = (C.c_void_p * 6)(*fbs[:6])
    assert N.dev.yrtDenoiseCube(d.h, arr, 6, scene, fba, C.byref(p)) != 0 and "size" in d.error()
    assert N.dev.yrtDenoiseCube(d.h, None, 6, scene, fba, None) != 0 and "null" in d.error()
    assert N.dev.yrtDenoiseCube(d.h, arr, 6, None, fba, None) != 0 and "null" in d.error()


def test_pitched_rig_is_refused(host_device):
    """lookAt - origin not perpendicular to up: the reference turns the faces about axes that are not
    the frame's own, the faces no longer tile the sphere, and the call says so instead of filtering
    across the gaps."""
    args = cref.cube_args(16, 1)
    args[args.index("-vi") + 2] = "400"  # look upwards
    s = yrt.Session(args, device=host_device)
    cams = [s.camera(f) for f in range(12)]
    fbs = [host_device.rtNewFrameBuffer("RGB_FLOAT32", 16, 16) for _ in range(12)]
    with pytest.raises(RuntimeError, match="do not form a cube.*perpendicular") as e:
        host_device.denoise_cube(cams, s.info()["scene"], fbs)
    assert "host-only" not in str(e.value)
    s.close()


def test_denoise_cube_tag_parses(host_device):
    for v in ("0", "1"):
        yrt.Session(cref.cube_args(16, 1) + ["-denoise", "3", "-denoise-cube", v], device=host_device).close()
    yrt.Session(cref.cube_args(16, 1) + ["-denoise-cube", "1"], device=host_device).close()
    with pytest.raises(RuntimeError, match="-denoise-cube"):
        yrt.Session(cref.cube_args(16, 1) + ["-denoise-cube", "2"], device=host_device)


# ----------------------------------------------------------------------------- GPU
class Cube:
    """The 12-face job of the Cornell box seen from inside at one width and sample count; raw frames,
    guides, albedo and numpy expectations are computed once and shared (read-only)."""

    def __init__(self, dev, width, spp=4):
        self.dev, self.W = dev, width
        self.s = yrt.Session(cref.cube_args(width, spp), device=dev)
        i = self.s.info()
        self.scene, self.renderer, self.tm = i["scene"], i["renderer"], i["tonemapper"]
        self.cams = [self.s.camera(f) for f in range(12)]
        self._raw, self._expect = {}, {}
        self._guides = self._albedo = None

    def job(self, fmt, faces=range(12)):
        """Fresh framebuffers holding the faces' frames, not mapped yet."""
        fbs = [self.dev.rtNewFrameBuffer(fmt, self.W, self.W) for _ in faces]
        self.dev.rtRenderFrames(self.renderer, [self.cams[f] for f in faces], self.scene, self.tm, fbs, 0)
        return fbs

    def read(self, fbs, fmt):
        """(faces, W, stride) uint8: the mapped bytes, row padding included."""
        return np.stack([mapped(self.dev, fb, fmt, self.W, self.W) for fb in fbs])

    def px(self, raw, fmt):
        return np.stack([pixels(r, fmt, self.W) for r in raw])

    def raw(self, fmt):
        if fmt not in self._raw:
            self._raw[fmt] = self.read(self.job(fmt), fmt)
        return self._raw[fmt]

    def guides(self):
        if self._guides is None:
            g = [self.dev.render_guides(c, self.scene, self.W, self.W) for c in self.cams]
            self._guides = np.stack([a for a, _ in g]), np.stack([b for _, b in g])
        return self._guides

    def hit(self):
        return np.isfinite(self.guides()[0][..., 3])

    def albedo(self):
        if self._albedo is None:
            self._albedo = np.stack([self.dev.render_albedo(c, self.scene, self.W, self.W) for c in self.cams])
        return self._albedo

    def denoised(self, fmt, faces=range(12), **kw):
        fbs = self.job(fmt, faces)
        self.dev.denoise_cube([self.cams[f] for f in faces], self.scene, fbs, **kw)
        return self.read(fbs, fmt)

    def expect(self, fmt, iterations, demodulate=False):
        """The numpy cube filter on the GPU's own raw frames and per-face guides: (12, W, W, 3)."""
        key = (fmt in ("RGB8", "RGBA8"), iterations, demodulate)
        if key not in self._expect:
            p = self.px(self.raw(fmt), fmt)[..., :3]
            c0 = p.astype(np.float64) / 255.0 if p.dtype == np.uint8 else p.astype(np.float64)
            pos, nrm = self.guides()
            eyes = []
            for e in range(2):
                sel = slice(6 * e, 6 * e + 6)
                if demodulate:
                    eyes.append(cref.demodulated_atrous_cube(c0[sel], pos[sel], nrm[sel], self.albedo()[sel], iterations,
                                                             POWER, FLOOR, **DEFAULTS))
                else:
                    eyes.append(cref.atrous_cube(c0[sel], pos[sel], nrm[sel], iterations, **DEFAULTS))
            self._expect[key] = np.concatenate(eyes)
        return self._expect[key]


@pytest.fixture(scope="module")
def cube(gpu_device):
    return Cube(gpu_device, W)


@pytest.fixture(scope="module")
def cube8(gpu_device):
    return Cube(gpu_device, W8)


@pytest.mark.gpu
def test_scene_has_hits_and_misses(cube):
    hit = cube.hit()
    assert all(hit[f].sum() > W * W // 4 for f in range(12)), [int(h.sum()) for h in hit]
    assert sum(int((~hit[f]).sum() > 50) for f in range(6)) >= 2, "the open front must show on two faces per eye"
    assert (cube.px(cube.raw("RGB_FLOAT32"), "RGB_FLOAT32").max(-1) > 0.01).mean() > 0.2, "the scene must be lit"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_cube_filter_matches_numpy(cube, fmt, iterations):
    """|gpu - numpy| / max(|numpy|, 1/255) on hit pixels, bound 1e-4 (FILTER_BOUND). Measured on an
    MI355X: 2.71e-6, 4.15e-6, 6.92e-6 for 1, 3, 5 iterations. Step 16 of the fifth iteration sends
    taps more than half a 48-pixel face deep into the neighbours."""
    raw = cube.px(cube.raw(fmt), fmt)
    got = cube.px(cube.denoised(fmt, iterations=iterations), fmt)
    want = cube.expect(fmt, iterations)
    hit = cube.hit()
    dev = reldev(got[..., :3][hit], want[hit])
    print(f"cube filter {fmt} x{iterations}: relative deviation {dev:.3g}")
    assert np.abs(got[..., :3][hit].astype(np.float64) - raw[..., :3][hit]).max() > 1e-3, "the filter must act"
    assert dev <= FILTER_BOUND
    assert np.array_equal(got[~hit].view(np.uint32), raw[~hit].view(np.uint32))
    if fmt == "RGBA_FLOAT32":
        assert np.array_equal(got[..., 3], raw[..., 3])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
def test_cube_filter_demodulated_matches_numpy(cube, fmt):
    """demodulate = 1, albedo_power = 1 / 2.2: the derived 1.4e-4 (DEMOD_BOUND); measured 2.55e-6."""
    raw = cube.px(cube.raw(fmt), fmt)
    got = cube.px(cube.denoised(fmt, demodulate=1, albedo_power=POWER), fmt)
    want = cube.expect(fmt, 5, demodulate=True)
    hit = cube.hit()
    dev = reldev(got[..., :3][hit], want[hit])
    print(f"cube filter {fmt} demodulated: relative deviation {dev:.3g}")
    assert dev <= DEMOD_BOUND
    assert np.array_equal(got[~hit].view(np.uint32), raw[~hit].view(np.uint32))
    plain = cube.px(cube.denoised(fmt), fmt)
    assert not np.array_equal(plain, got)


@pytest.mark.gpu
def test_cube_filter_rgb8(cube8):
    """Width 38: bytes within 1 of the quantized numpy result, the two padding bytes of every row and
    the miss pixels untouched."""
    d, fmt = cube8.dev, "RGB8"
    fbs = cube8.job(fmt)
    raw = cube8.read(fbs, fmt)
    raw[:, :, 3 * W8:] = 0xA5  # mark the padding, so that a store into it shows
    for fb, r in zip(fbs, raw):
        mapped(d, fb, fmt, W8, W8, write=r)
    d.denoise_cube(cube8.cams, cube8.scene, fbs)
    out = cube8.read(fbs, fmt)
    got, before = cube8.px(out, fmt), cube8.px(raw, fmt)
    assert np.array_equal(cube8.px(cube8.raw(fmt), fmt), before)
    want = ref.quantize(cube8.expect(fmt, 5))
    hit = cube8.hit()
    diff = np.abs(got[hit].astype(int) - want[hit].astype(int))
    print(f"cube filter RGB8: {float((diff > 0).mean()):.4f} of the bytes differ by 1, max {diff.max()}")
    assert diff.max() <= 1
    assert (got[hit] != before[hit]).mean() > 0.2, "the filter must act"
    assert np.array_equal(got[~hit], before[~hit])
    assert np.all(out[:, :, 3 * W8:] == 0xA5)
    # the frames filtered where they were rendered (in HBM) hold the same pixels
    assert np.array_equal(cube8.px(cube8.denoised(fmt), fmt), got)


@pytest.mark.gpu
def test_interior_is_the_per_face_filter(cube):
    """3 iterations reach 2 (1 + 2 + 4) = 14 pixels: a pixel at least 14 from every border has no tap
    chain that leaves its face, and equals yrtDenoiseFrameBuffer's result bit for bit; the border
    band differs."""
    fmt, R = "RGB_FLOAT32", 14
    d = cube.dev
    fbs = cube.job(fmt)
    for cam, fb in zip(cube.cams, fbs):
        d.denoise(cam, cube.scene, fb, iterations=3)
    per_face = cube.px(cube.read(fbs, fmt), fmt)
    whole = cube.px(cube.denoised(fmt, iterations=3), fmt)
    assert np.array_equal(per_face[:, R:W - R, R:W - R].view(np.uint32), whole[:, R:W - R, R:W - R].view(np.uint32))
    differs = [not np.array_equal(per_face[f], whole[f]) for f in range(12)]
    assert any(differs)
    print(f"faces whose border band differs from the per-face filter: {sum(differs)} of 12")


@pytest.mark.gpu
def test_eyes_are_independent(cube):
    fmt = "RGB_FLOAT32"
    both = cube.denoised(fmt, iterations=3)
    left = cube.denoised(fmt, range(0, 6), iterations=3)
    right = cube.denoised(fmt, range(6, 12), iterations=3)
    assert np.array_equal(both[:6], left) and np.array_equal(both[6:], right)
    # and the order of the faces in the call does not matter
    order = [7, 3, 0, 11, 5, 2, 9, 1, 6, 10, 4, 8]
    shuffled = cube.denoised(fmt, order, iterations=3)
    assert np.array_equal(shuffled, both[order])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGBA_FLOAT32"])
def test_constant_frame_stays_constant(cube, fmt):
    """Written through the mapped pixels (the upload path): every hit pixel keeps the value exactly
    (the kernel adds sum w (c_q - c_p) / sum w = 0), whatever the misses hold; misses and alpha are
    untouched."""
    d = cube.dev
    fbs = cube.job(fmt)
    hit = cube.hit()
    value = np.float32([0.7231, 0.05, 3.5])
    px = cube.px(cube.read(fbs, fmt), fmt).copy()
    px[..., :3] = np.float32(9.0)
    px[hit, :3] = value
    if fmt == "RGBA_FLOAT32":
        px[..., 3] = np.float32(0.25)
    for fb, p in zip(fbs, px):
        mapped(d, fb, fmt, W, W, write=p.view(np.uint8).reshape(W, -1))
    d.denoise_cube(cube.cams, cube.scene, fbs)
    out = cube.px(cube.read(fbs, fmt), fmt)
    assert np.array_equal(out[hit][:, :3], np.broadcast_to(value, out[hit][:, :3].shape))
    assert np.array_equal(out[~hit], px[~hit])
    if fmt == "RGBA_FLOAT32":
        assert np.all(out[..., 3] == np.float32(0.25))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB8", "RGB_FLOAT32", "RGBA_FLOAT32"])
def test_cube_zero_iterations_write_nothing(cube8, fmt):
    fbs = cube8.job(fmt)
    raw = cube8.read(fbs, fmt)
    cube8.dev.denoise_cube(cube8.cams, cube8.scene, fbs, iterations=0)
    assert np.array_equal(cube8.read(fbs, fmt), raw)
    # and on frames not mapped yet (the RGB8 padding of a frame in HBM is whatever the block held)
    assert np.array_equal(cube8.px(cube8.denoised(fmt, iterations=0), fmt), cube8.px(raw, fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["RGB8", "RGB_FLOAT32", "RGBA_FLOAT32"])
def test_cube_is_filtered_where_it_lives(cube8, fmt):
    """Filtered before the first map (RGB8 / RGB_FLOAT32: in the frame block), after a map (uploaded),
    or with half of the faces mapped: the same pixels."""
    d = cube8.dev
    first = cube8.px(cube8.denoised(fmt, iterations=3), fmt)
    for some in (range(12), range(0, 12, 2)):
        fbs = cube8.job(fmt)
        for k in some:
            mapped(d, fbs[k], fmt, W8, W8)
        d.denoise_cube(cube8.cams, cube8.scene, fbs, iterations=3)
        second = cube8.px(cube8.read(fbs, fmt), fmt)
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8))
    assert not np.array_equal(first, cube8.px(cube8.raw(fmt), fmt))


@pytest.mark.gpu
def test_denoise_times_report_the_cube_call(cube):
    d = cube.dev
    d.set_kernel_timing(True)
    try:
        cube.denoised("RGB_FLOAT32", iterations=2)
        g, f = d.denoise_times()
    finally:
        d.set_kernel_timing(False)
    assert 0 < g < 100 and 0 < f < 100


@pytest.mark.gpu
def test_cube_filter_removes_the_seam(gpu_device):
    """Left eye, 64 x 64 faces, 4 spp against 1024 spp, gamma 2.2, default weights, 5 iterations, over
    the hit pixels below 1 in both frames. The cube filter's seam error (denoise_cube_ref.seam_error)
    and its mean squared error over the one-pixel border band are both strictly below the per-face
    filter's.

    CPU rehearsal with the final rule (tools/denoise_cube_rehearsal.py: the oracle's frames, which
    the GPU's equal bit for bit, guides from the oracle's camera rays with geometric normals, the
    numpy filters): seam error raw 0.108023, per-face 0.0518634, cube 0.0204186 (ratio 0.3937);
    band mean squared error per-face 0.00646856, cube 0.00592287 (ratio 0.9156). The seam ratio's
    bound lies halfway between the rehearsed ratio and 1: (0.3937 + 1) / 2 = 0.697."""
    S, d = 64, gpu_device
    conv_cube = Cube(d, S, 1024)
    conv = conv_cube.px(conv_cube.read(conv_cube.job("RGB_FLOAT32", range(6)), "RGB_FLOAT32"), "RGB_FLOAT32")
    conv = conv.astype(np.float64)
    conv_cube.s.close()
    c = Cube(d, S, 4)
    fmt, left = "RGB_FLOAT32", range(6)
    raw = c.px(c.read(c.job(fmt, left), fmt), fmt).astype(np.float64)
    fbs = c.job(fmt, left)
    for f in left:
        d.denoise(c.cams[f], c.scene, fbs[f])
    per_face = c.px(c.read(fbs, fmt), fmt).astype(np.float64)
    whole = c.px(c.denoised(fmt, left), fmt).astype(np.float64)
    hit = np.stack([np.isfinite(d.render_guides(c.cams[f], c.scene, S, S)[0][..., 3]) for f in left])
    c.s.close()
    ok = hit & (conv.max(-1) < 1) & (raw.max(-1) < 1)
    seam = {n: cref.seam_error(x, conv, ok) for n, x in (("raw", raw), ("per-face", per_face), ("cube", whole))}
    band = {n: cref.band_mse(x, conv, ok, 1) for n, x in (("raw", raw), ("per-face", per_face), ("cube", whole))}
    print(f"seam error {seam}, ratio {seam['cube'] / seam['per-face']:.4f}; one-pixel band mse {band}, "
          f"ratio {band['cube'] / band['per-face']:.4f}; {ok.mean():.4f} of the pixels count")
    assert seam["cube"] < seam["per-face"] < seam["raw"]
    assert band["cube"] < band["per-face"]
    assert seam["cube"] <= 0.697 * seam["per-face"]


@pytest.mark.gpu
@pytest.mark.parametrize("albedo", [False, True])
def test_command_line_cube(cube, albedo):
    """-denoise 3 -denoise-cube 1: render_cube equals the API call on the same job bit for bit;
    without the tag (or with 0) it equals the loop of per-face calls."""
    d, fmt = cube.dev, "RGB_FLOAT32"
    kw = dict(iterations=3, demodulate=1, albedo_power=POWER) if albedo else dict(iterations=3)
    extra = ["-denoise-albedo", "1"] if albedo else []

    def session(*tags):
        s = yrt.Session(cref.cube_args(W, 4) + ["-fb", fmt, "-denoise", "3"] + extra + list(tags), device=d)
        faces = np.stack(s.render_cube())
        s.close()
        return faces

    api = cube.px(cube.denoised(fmt, **kw), fmt)
    assert np.array_equal(session("-denoise-cube", "1").view(np.uint32), api.view(np.uint32))
    fbs = cube.job(fmt)
    for cam, fb in zip(cube.cams, fbs):
        d.denoise(cam, cube.scene, fb, **kw)
    loop = cube.px(cube.read(fbs, fmt), fmt)
    assert np.array_equal(session().view(np.uint32), loop.view(np.uint32))
    assert np.array_equal(session("-denoise-cube", "0").view(np.uint32), loop.view(np.uint32))
    assert not np.array_equal(api, loop)
