"""The variance-guided denoiser on the host ("variance-guided"): the variance estimate
(csrc/common/yrt_pixel_variance.h through yrtDebugFrameVariance, the header k_frame_variance
compiles) against its numpy restatements on the oracle's sums, the grown parameter struct's size
rule and refusals, the front end's -denoise-variance tag, the built kernels' metadata, and the numpy
filter itself (tests/denoise_variance_ref.py) on the oracle's frames."""
from __future__ import annotations

import ctypes as C
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest

import yrt
from yrt import _native as N

import denoise_ref as ref
import denoise_variance_ref as vref
from adaptive_ref import sums_after
from helpers import SCENES, c1_args, c2_args
from trace_scenes import MeshScene

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from code_object_resources import DEFAULT_LIB, LLVM, kernel_resources  # noqa: E402

OLD_SIZE = 32  # sizeof(YRTDenoiseParams) before the variance-guided fields
# name -> (session arguments, width, height, iteration counts): a frame with partial tiles after an
# even, an odd (unequal halves: 2 against 1 iterations) and a larger count, and C2
FRAMES = {
    "C1": (["-c", str(SCENES / "cornell_box.ecs"), "-size", "40", "24", "-spp", "4"], 40, 24, (2, 3, 8)),
    "C2": (c2_args(48, 4), 48, 48, (2,)),
}


@pytest.fixture(scope="module")
def frame_sums(host_device):
    """name -> {n: (accu, half)}: the oracle's sums after n iterations. Shared: not modified."""
    out = {}
    for name, (args, w, h, counts) in FRAMES.items():
        s = yrt.Session(args, device=host_device)
        blob = s.export_frame()
        s.close()
        out[name] = {n: sums_after(blob, w, h, n) for n in counts}
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("name", list(FRAMES))
def test_estimate_equals_the_restatement(frame_sums, name):
    """yrt.frame_variance (gamma 1, no vignette) against denoise_variance_ref.frame_variance_f32, bit
    for bit; the factor is 1/4 for equal halves and 2/9 after three iterations."""
    for n, (accu, half) in frame_sums[name].items():
        got, want = yrt.frame_variance(accu, half), vref.frame_variance_f32(accu, half)
        assert got.shape == accu.shape and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(want)), (name, n)
        assert (got[..., 3] == 1).all() and np.isfinite(got).all() and (got[..., :3] >= 0).all()
        assert (got[..., :3] > 0).mean() > 0.5, "the halves must differ"
        f64 = vref.frame_variance_f64(accu, half)
        lit = f64[..., :3] > 1e-12
        assert np.abs(got[..., :3][lit] / f64[..., :3][lit] - 1).max() < 1e-3
        _, _, f = vref.display_halves_f64(accu, half)
        assert np.allclose(f, 0.25 if n % 2 == 0 else (n // 2 + 1) * (n // 2) / n ** 2)
    if len(frame_sums[name]) > 1:
        a, b = list(frame_sums[name].values())[:2]
        assert not np.array_equal(yrt.frame_variance(*a), yrt.frame_variance(*b))


@pytest.mark.parametrize("vignetting", [False, True])
@pytest.mark.parametrize("name", list(FRAMES))
def test_estimate_with_gamma_against_float64(frame_sums, name, vignetting):
    """Gamma 2.2 (and the vignette): the header against the float64 definition within
    denoise_variance_ref.frame_variance_bound, derived there from the accuracy of powf, cosf and the
    reference's rcp, not tuned."""
    for n, (accu, half) in frame_sums[name].items():
        got = yrt.frame_variance(accu, half, 2.2, vignetting).astype(np.float64)
        want = vref.frame_variance_f64(accu, half, 2.2, vignetting)
        bound = vref.frame_variance_bound(accu, half, 2.2, vignetting)
        ratio = np.abs(got[..., :3] - want[..., :3]) / bound
        rel = np.abs(got[..., :3] - want[..., :3]) / np.maximum(want[..., :3], vref.FLOOR)
        print(f"{name} after {n}, vignette {vignetting}: worst |v - v64| / bound {ratio.max():.3g}, "
              f"|v - v64| / max(v64, floor) {rel.max():.3g}")
        assert (ratio <= 1).all(), (name, n, ratio.max())
        # the bound in the filter's own measure: it allows the 2e-5 of powf on both halves where they
        # nearly cancel; beyond a tenth of what the weight's denominator holds it would check nothing
        width = bound / np.maximum(want[..., :3], vref.FLOOR)
        assert width.max() <= 0.1, width.max()
        assert not np.array_equal(got, yrt.frame_variance(accu, half).astype(np.float64))


def test_hand_made_pixels():
    """A half without samples (h = 0, or r = 0), a non-finite sum and S_c < H_c: the variance is 0
    where it is not finite, and max(S - H, 0) clamps."""
    accu = np.zeros((2, 3, 4), np.float32)
    half = np.zeros_like(accu)
    accu[...] = (2.0, 4.0, 6.0, 8.0)
    half[...] = (1.0, 1.0, 3.0, 4.0)
    half[0, 1, 3] = 0.0                      # no even iteration
    half[0, 2] = accu[0, 2]                  # no odd iteration
    accu[1, 0, 0] = np.inf
    half[1, 1, :3] = (3.0, 1.0, 3.0)         # H_r > S_r
    got, want = yrt.frame_variance(accu, half), vref.frame_variance_f32(accu, half)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(got).all()
    # A = (.25, .25, .75), B = (.25, .75, .75), f = 1/4
    assert np.allclose(got[0, 0], (0.0, 0.0625, 0.0, 1.0), atol=1e-6)
    assert (got[0, 1, :3] == 0).all() and (got[0, 2, :3] == 0).all() and got[1, 0, 0] == 0
    assert abs(float(got[1, 1, 0]) - 0.75 ** 2 / 4) < 1e-6
    with pytest.raises(ValueError):
        yrt.frame_variance(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 3), np.float32))


# ----------------------------------------------------------------------------- the struct
def test_denoise_params_grow_by_size(host_device):
    full = C.sizeof(N.DenoiseVarianceParams)
    assert C.sizeof(N.DenoiseParams) == OLD_SIZE and full == OLD_SIZE + 12
    p = N.DenoiseVarianceParams(size=full, varianceGuided=-7, sigmaVariance=-7, varianceFloor=-7)
    short = C.cast(C.pointer(p), C.POINTER(N.DenoiseParams))
    assert N.dev.yrtDenoiseDefaults(short) == 0
    assert (p.varianceGuided, p.varianceFloor) == (0, vref.FLOOR)
    assert p.sigmaVariance in (1.0, 2.0, 3.0, 4.0)
    assert yrt.Device.denoise_defaults(variance=True)["sigma_variance"] == p.sigmaVariance
    p = N.DenoiseVarianceParams(size=OLD_SIZE, varianceGuided=-7, sigmaVariance=-7, varianceFloor=-7)
    assert N.dev.yrtDenoiseDefaults(C.cast(C.pointer(p), C.POINTER(N.DenoiseParams))) == 0
    assert (p.iterations, p.demodulate) == (5, 0)
    assert (p.varianceGuided, p.sigmaVariance, p.varianceFloor) == (-7, -7, -7)

    ms = MeshScene(host_device, ref.two_quads(), eye=(0, 0, 0), look=(0, 0, 1))
    fb = host_device.rtNewFrameBuffer("RGB_FLOAT32", 8, 8)

    def call(p):
        rc = N.dev.yrtDenoiseFrameBuffer(host_device.h, ms.camera, ms.scene, fb,
                                         C.cast(C.pointer(p), C.POINTER(N.DenoiseParams)))
        return rc, host_device.error()

    # the previous header's struct is accepted as it is (the call then meets the host-only device)
    rc, err = call(N.DenoiseParams(size=OLD_SIZE, iterations=1, sigmaColor=1, sigmaNormal=64, sigmaPosition=0.02,
                                   demodulate=0, albedoPower=1, albedoFloor=1 / 255))
    assert rc != 0 and "host-only" in err
    base = dict(size=full, iterations=1, sigmaColor=1, sigmaNormal=64, sigmaPosition=0.02, demodulate=0, albedoPower=1,
                albedoFloor=1 / 255)
    # the new fields are judged only when the mode is set
    for bad in (dict(sigmaVariance=0.0, varianceFloor=vref.FLOOR), dict(sigmaVariance=float("nan"), varianceFloor=vref.FLOOR),
                dict(sigmaVariance=float("inf"), varianceFloor=vref.FLOOR), dict(sigmaVariance=2.0, varianceFloor=0.0),
                dict(sigmaVariance=2.0, varianceFloor=-1.0), dict(sigmaVariance=2.0, varianceFloor=float("nan"))):
        rc, err = call(N.DenoiseVarianceParams(varianceGuided=1, **base, **bad))
        assert rc != 0 and "varianceGuided" in err and "host-only" not in err, (bad, err)
        rc, err = call(N.DenoiseVarianceParams(varianceGuided=0, **base, **bad))
        assert rc != 0 and "host-only" in err, (bad, err)
    # a struct that ends before the fields does not have them read
    p = N.DenoiseVarianceParams(varianceGuided=1, sigmaVariance=-1, varianceFloor=-1, **{**base, "size": OLD_SIZE})
    rc, err = call(p)
    assert rc != 0 and "host-only" in err
    with pytest.raises(RuntimeError, match="host-only"):
        host_device.denoise(ms.camera, ms.scene, fb, variance_guided=1)
    with pytest.raises(RuntimeError, match="host-only"):
        host_device.frame_variance(fb)


def test_defaults_keys_are_unchanged():
    """The earlier dictionaries keep their keys; the new fields come with variance=True."""
    d = yrt.Device.denoise_defaults(extended=True)
    assert "variance_guided" not in d and set(yrt.Device.denoise_defaults()) < set(d)
    v = yrt.Device.denoise_defaults(variance=True)
    assert v["variance_guided"] == 0 and v["variance_floor"] == vref.FLOOR


# ----------------------------------------------------------------------------- the front end
def test_denoise_variance_tag(host_device):
    base = c1_args(16)
    for tags in (["-adaptive", "0", "2", "-denoise", "5", "-denoise-variance", "1"],
                 ["-denoise-variance", "1", "-denoise", "5", "-adaptive", "0", "2"]):  # any order
        s = yrt.Session(base + tags, device=host_device)
        p = s.denoise_params()
        s.close()
        assert p["iterations"] == 5 and p["varianceGuided"] == 1 and p["demodulate"] == 0
        assert p["sigmaVariance"] == yrt.Device.denoise_defaults(variance=True)["sigma_variance"]
        assert p["varianceFloor"] == vref.FLOOR
    s = yrt.Session(base + ["-adaptive", "0", "2", "-denoise", "3", "-denoise-variance", "1", "-denoise-albedo", "1",
                            "-gamma", "2.2"], device=host_device)
    p = s.denoise_params()
    s.close()
    assert (p["varianceGuided"], p["demodulate"], p["iterations"]) == (1, 1, 3)
    assert p["albedoPower"] == float(np.float32(1 / 2.2))
    for tags in (["-denoise", "3"], ["-denoise", "3", "-denoise-variance", "0"],
                 ["-adaptive", "0", "2", "-denoise", "3", "-denoise-variance", "0"]):
        s = yrt.Session(base + tags, device=host_device)
        p = s.denoise_params()
        s.close()
        assert p["iterations"] == 3 and "varianceGuided" not in p  # the struct ends after `iterations`
    with pytest.raises(RuntimeError, match="-denoise-variance 1 needs -adaptive"):
        yrt.Session(base + ["-denoise", "3", "-denoise-variance", "1"], device=host_device)
    with pytest.raises(RuntimeError, match="-denoise-variance"):
        yrt.Session(base + ["-adaptive", "0", "2", "-denoise-variance", "2"], device=host_device)


def test_denoise_variance_tag_in_ecs(host_device, tmp_path):
    ecs = tmp_path / "variance.ecs"
    ecs.write_text(f"-c {SCENES / 'cornell_box.ecs'}\n-size 16 16\n-adaptive 0 2\n-denoise 4\n-denoise-variance 1\n")
    s = yrt.Session(["-c", str(ecs)], device=host_device)
    p = s.denoise_params()
    s.close()
    assert (p["iterations"], p["varianceGuided"]) == (4, 1)


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.skipif(not DEFAULT_LIB.exists() or not (LLVM / "clang-offload-bundler").exists()
                    or shutil.which("c++filt") is None, reason="device library not built or ROCm LLVM tools absent")
def test_variance_kernels_in_the_code_object():
    res = kernel_resources(DEFAULT_LIB)

    def named(prefix):
        return {k: v for k, v in res.items() if k.startswith(f"void yrt::{prefix}") or k.startswith(f"yrt::{prefix}")}

    family = {"k_atrous_load_var<": 2, "k_atrous_var<": 4, "k_frame_variance": 1}
    found = {p: named(p) for p in family}
    assert {p: len(v) for p, v in found.items()} == family, {p: sorted(v) for p, v in found.items()}
    for p, kernels in found.items():
        for name, r in kernels.items():
            assert r["scratch"] == 0, (name, r)


# ----------------------------------------------------------------------------- the numpy filter
def _plane(h=12, w=16):
    """Guides of a plane z = 3 facing a camera at the origin, with a band of misses."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pos4 = np.stack([(xx - w / 2) * 0.1, (yy - h / 2) * 0.1, np.full((h, w), 3.0), np.full((h, w), 3.0)], -1)
    nrm4 = np.zeros((h, w, 4))
    nrm4[..., 2], nrm4[..., 3] = -1.0, 1.0
    pos4[:, 5] = (0, 0, 0, np.inf)
    nrm4[:, 5] = 0
    return pos4, nrm4


def test_filter_keeps_a_constant_frame_with_zero_variance():
    pos4, nrm4 = _plane()
    hit = np.isfinite(pos4[..., 3])
    c0 = np.zeros(hit.shape + (3,))
    c0[hit] = (0.7231, 0.05, 3.5)
    c0[~hit] = 9.0
    var4 = np.zeros(hit.shape + (4,))
    c, v = vref.atrous_var(c0, var4, pos4, nrm4, 5, 3.0, vref.FLOOR, 64.0, 0.02, return_variance=True)
    assert np.abs(c[hit] - c0[hit]).max() <= 1e-15 and np.array_equal(c[~hit], c0[~hit])
    assert (v == 0).all()


def test_filter_follows_the_variance():
    """A step of height 0.2 on a flat plane, no noise. With zero variance the weight's width is the
    floor, 1/255: the step survives five iterations. With a variance of 0.01 per pixel (a standard
    deviation of half the step) and sigmaVariance 3 the filter blurs it, and the filtered variance
    falls below the input's everywhere."""
    pos4, nrm4 = _plane()
    hit = np.isfinite(pos4[..., 3])
    c0 = np.zeros(hit.shape + (3,))
    c0[:, 9:] = 0.2
    quiet = np.zeros(hit.shape + (4,))
    kept = vref.atrous_var(c0, quiet, pos4, nrm4, 5, 3.0, vref.FLOOR, 64.0, 0.02)
    assert np.abs(kept - c0)[hit].max() < 1e-6
    noisy = np.zeros(hit.shape + (4,))
    noisy[..., :3] = 0.01 / 3
    blurred, v = vref.atrous_var(c0, noisy, pos4, nrm4, 5, 3.0, vref.FLOOR, 64.0, 0.02, return_variance=True)
    # the first iteration's weight across the step is exp(-0.12 / 0.09) = 0.26; later ones see less variance
    assert np.abs(blurred - c0)[hit].max() > 5e-3
    assert (v[hit] < 0.01).all() and (v[hit] > 0).all() and (v[~hit] == 0).all()
    # and a demodulated frame is the plain one when the modulation is 1
    m = np.ones(hit.shape + (3,))
    assert np.array_equal(vref.atrous_var(c0, noisy, pos4, nrm4, 3, 3.0, vref.FLOOR, 64.0, 0.02, m=m),
                          vref.atrous_var(c0, noisy, pos4, nrm4, 3, 3.0, vref.FLOOR, 64.0, 0.02))


def test_default_beats_the_plain_filter_on_c1():
    """The oracle's C1 64 x 64 frame of 2 iterations of 4 spp against its 1024-spp frame
    (tools/denoise_variance_rehearsal.py): the variance-guided filter at the library's default
    sigmaVariance has a lower whole-frame and a lower below-1 mean squared error than the plain
    default filter, each by more than 10 %, and a lower whole-frame error than the raw frame. The
    inequality tests/test_denoise_variance.py repeats on the device. Rehearsal: whole frame 0.671
    against 0.988, below 1 0.220 against 0.355."""
    import denoise_variance_rehearsal as tool
    raw, conv, plain, guided = tool.cpu_filters("C1", 64, 2)
    d = yrt.Device.denoise_defaults(variance=True)
    pw, pb = vref.mse_ratios(plain(d["sigma_color"]), raw, conv)
    gw, gb = vref.mse_ratios(guided(d["sigma_variance"]), raw, conv)
    print(f"C1 64x64, 2 x 4 spp: plain whole {pw:.4f} below-1 {pb:.4f}; variance-guided whole {gw:.4f} below-1 {gb:.4f}")
    assert gw < 0.9 * pw and gb < 0.9 * pb and gw < 1.0
