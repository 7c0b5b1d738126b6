"""Adaptive sampling on the host: the tile error estimate (csrc/common/yrt_tile_error.h through
yrtDebugTileError, the header the kernel k_tile_error compiles) against a numpy restatement of its
operation sequence bit for bit and against float64 arithmetic within a derived bound, on the
oracle's own sums; and what yrtRenderAdaptive refuses before it launches anything.
"""
import numpy as np
import pytest

import yrt
from adaptive_ref import U, pixel_error, sums_after, tile_error, tile_error_f64
from helpers import SCENES, c1_args

# name -> (session arguments, width, height): C1 with whole tiles, and a frame with partial tiles
# on both edges (40 = 2 * 16 + 8, 24 = 16 + 8)
FRAMES = {
    "C1": (c1_args(64, 4), 64, 64),
    "partial": (["-c", str(SCENES / "cornell_box.ecs"), "-size", "40", "24", "-spp", "4"], 40, 24),
}
CHECKS = (2, 4)  # iterations after which the sums are compared


@pytest.fixture(scope="module")
def frame_sums(host_device):
    """name -> {n: (accu, half)}: the oracle's sums after n iterations. Shared: not modified."""
    out = {}
    for name, (args, w, h) in FRAMES.items():
        s = yrt.Session(args, device=host_device)
        blob = s.export_frame()
        s.close()
        out[name] = {n: sums_after(blob, w, h, n) for n in CHECKS}
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(FRAMES))
def test_estimate_equals_the_restatement(frame_sums, name):
    """yrtDebugTileError against adaptive_ref.tile_error (numpy float32, rcp / rsqrt from
    oracle.vecmath, the pairwise tree by reshapes), bit for bit, on the oracle's sums."""
    _, w, h = FRAMES[name]
    for n in CHECKS:
        accu, half = frame_sums[name][n]
        got, want = yrt.tile_error(accu, half), tile_error(accu, half)
        assert got.shape == ((h + 15) // 16, (w + 15) // 16) == want.shape
        assert np.isfinite(want).all() and (want > 0).any()
        assert np.array_equal(_bits(got), _bits(want)), (name, n, got, want)
    a, b = (yrt.tile_error(*frame_sums[name][n]) for n in CHECKS)
    assert not np.array_equal(a, b), "the estimate does not depend on the iteration count"


def test_hand_made_pixels():
    """One 16 x 16 tile, every pixel I = A = (.25, .5, .75) (e = 0) but for: a black pixel (s = 0 ->
    e = 0, no 0 * inf), a NaN channel (s is NaN, not > 0 -> e = 0), an infinite channel (d = inf,
    rsqrt(inf) = 0 -> e = NaN and with it the tile), and a plain differing pixel."""
    base = np.zeros((16, 16, 4), np.float32)
    base[...] = (1.0, 2.0, 3.0, 4.0)
    half = np.zeros_like(base)
    half[...] = (0.5, 1.0, 1.5, 2.0)
    assert yrt.tile_error(base, half)[0, 0] == 0.0 and tile_error(base, half)[0, 0] == 0.0  # I = A
    cases = {}
    a = base.copy(); a[3, 5, :3] = 0; h = half.copy(); h[3, 5, :3] = 0
    cases["black"] = (a, h, 0.0)
    a = base.copy(); a[0, 0, 1] = np.nan
    cases["nan"] = (a, half, 0.0)
    a = base.copy(); a[15, 15, 2] = np.inf
    cases["inf"] = (a, half, np.nan)
    a = base.copy(); a[7, 9, :3] = (2.0, 2.0, 3.0)  # I = (.5, .5, .75): d = .25, s = 1.75
    cases["differs"] = (a, half, None)
    for name, (a, h, want) in cases.items():
        got, ref = yrt.tile_error(a, h), tile_error(a, h)
        assert np.array_equal(_bits(got), _bits(ref)), (name, got, ref)
        if want is not None:
            assert (np.isnan(got[0, 0]) if np.isnan(want) else got[0, 0] == want), (name, got)
    e = pixel_error(cases["differs"][0], half)
    assert np.count_nonzero(e) == 1 and abs(float(e[7, 9]) - 0.25 / np.sqrt(1.75)) < 1e-6
    assert abs(float(yrt.tile_error(cases["differs"][0], half)[0, 0]) - 0.25 / np.sqrt(1.75) / 256) < 1e-8
    # a NaN error is below no threshold, as the kernel's strict comparison reads it
    assert not (yrt.tile_error(*cases["inf"][:2])[0, 0] < np.float32(1e30))


@pytest.mark.parametrize("name", list(FRAMES))
def test_estimate_against_float64(frame_sums, name):
    """yrtDebugTileError against the formula in float64 (true division and square root) on the same
    float32 sums, within adaptive_ref.tile_error_f64's bound — derived here, not tuned. u = 2^-24.

    Per pixel and channel, with exact quotients I^ = S / w, A^ = H / h >= 0:
      I = fl(S * rcp(w)) = I^ (1 + r)(1 + d0), |r| <= 5 u (rcp, progressive_ref.mean_bound),
      so |I - I^| <= a I^, a = (1 + 5u)(1 + u) - 1, and the same for A.
    The difference cancels: fl(I - A) is off from I^ - A^ by at most a (I^ + A^)(1 + u) + u |I^ - A^|,
    an error that scales with the radiance, not with the difference. Summed over the channels (two
    more roundings):  |d - d^| <= a1 (s^ + sA^) + 3u d^,  a1 = a (1 + u)^3, s^ = sum I^, sA^ = sum A^.
    s = s^ (1 + th), |th| <= b = (1 + a)(1 + u)^2 - 1 (non-negative terms).
    rsqrt(s) = s^-1/2 (1 + rho), |rho| <= q = 8u: the estimate is within 1.5 * 2^-12, one Newton step
    leaves 1.5 eps^2 + .5 eps^3 <= 3.4u, and its five rounded operations add (1.5 + 1.5 + 1) u.
    e = fl(d * rsqrt(s)) = d / sqrt(s^) (1 + eta), |eta| <= c = (1 + q)(1 + u) / sqrt(1 - b) - 1, so
      |e - e^| <= (1 + c) a1 (s^ + sA^) / sqrt(s^) + (c + 3u (1 + c)) e^      (+ tiny below 2^-126).
    The tile: 256 non-negative slots through eight tree levels, times rcp(n_T) (5u) and one product:
      |E - E^| <= (1 + t) mean|e - e^| + t E^,  t = (1 + u)^8 (1 + 5u)(1 + u) - 1."""
    for n in CHECKS:
        accu, half = frame_sums[name][n]
        got = yrt.tile_error(accu, half).astype(np.float64)
        E, bound = tile_error_f64(accu, half)
        ratio = np.abs(got - E) / bound
        print(f"{name} after {n} iterations: worst |E - E64| / bound = {ratio.max():.3f}, "
              f"bound / E up to {np.max(bound / np.maximum(E, 1e-300)):.2e}")
        assert (ratio <= 1.0).all(), (name, n, ratio.max())
        assert (bound <= 1e-2 * np.maximum(E, 1e-6)).all(), "a bound this wide checks nothing"
    assert U == 2.0 ** -24


def test_refusals(host_device):
    """The argument and state refusals, judged before the device is: a host-only device meets each
    for its own reason and the plain call for being host-only."""
    dev = host_device
    s = yrt.Session(c1_args(32, 1), device=dev)
    i = s.info()

    def call(d=dev, renderer=None, **kw):
        return d.rtRenderAdaptive(renderer or i["renderer"], s.camera(), i["scene"], i["tonemapper"],
                                  i["framebuffer"], **kw)

    try:
        with pytest.raises(RuntimeError, match="maxIterations must be at least 1"):
            call(threshold=0.1, max_iterations=0)
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(RuntimeError, match="threshold is not finite"):
                call(threshold=bad, max_iterations=4)
        dbg = dev.rtNewRenderer("debug")
        dev.rtCommit(dbg)
        with pytest.raises(RuntimeError, match="debug renderer"):
            call(renderer=dbg, threshold=0.1, max_iterations=4)
        dev.rtDecRef(dbg)
        dev.set_tile_shard(1, 2)
        try:
            with pytest.raises(RuntimeError, match="tile shard, communicator or hub is armed"):
                call(threshold=0.1, max_iterations=4)
        finally:
            dev.set_tile_shard(0, 1)
        dev.set_ray_capture(16)
        try:
            with pytest.raises(RuntimeError, match="ray capture is armed"):
                call(threshold=0.1, max_iterations=4)
        finally:
            dev.set_ray_capture(0)
        with pytest.raises(RuntimeError, match=r'host-only device \(created with parms "host"\)'):
            call(threshold=0.1, max_iterations=4)
        it, err = dev.adaptive_tiles(i["framebuffer"])
        assert it.size == 0 and err.size == 0  # no adaptive render yet
    finally:
        s.close()
    d = yrt.Device.adaptive_defaults()
    assert d["max_iterations"] >= 1 and d["min_iterations"] == 2 and np.isfinite(d["threshold"])
    with pytest.raises(ValueError):
        yrt.tile_error(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 3), np.float32))
