"""Adaptive sampling on the device: rtRenderAdaptive against the plain progressive sequence.

A tile that ran n iterations holds, bit for bit, what n calls of rtRenderFrame(..., accumulate=1)
leave there (a pixel's inputs do not depend on which tiles render with it), so the oracle's
progressive sequence (tests/progressive_ref.py) is an exact reference for every tile, whatever the
tiles around it did. The errors the device reports are the shared header's
(csrc/common/yrt_tile_error.h through yrt.tile_error) of the oracle's sums, bit for bit, and the
stop decisions follow from them (tests/adaptive_ref.py restates the earlier checks).

Thresholds: chosen on the CPU from the restated errors of the oracle's sums so that no active
tile's error lies within 1 % of the threshold at any check (each test asserts it):
  C1 64x64, 4 spp, 0.13, 8 iterations   closest 2.6 % (the float64 formula: 2.8 %); first choice
  C2 48x48, 4 spp, 0.13, 12 iterations  closest 3.6 %; one tile (the light's) stays near 0.4
  C1 40x24 (partial tiles), 0.13, 8     closest 11 %
  dof 24x18, 0.018, 8                   closest 6.3 % (0.02: 1.5 %, rejected)
  motion 40x40, 0.23, 8                 closest 4.6 % (0.22: 1.6 %, 0.24: 0.2 %, rejected)
"""
import numpy as np
import pytest

import yrt
from adaptive_ref import sums_after, tile_error
from helpers import SCENES, c1_args, c2_args
from progressive_ref import oracle_sequence
from test_progressive import SEQUENCES, Progressive, _same

pytestmark = pytest.mark.gpu

# name -> (session arguments, threshold, maxIterations)
CASES = {
    "C1": (lambda: c1_args(64, 4), 0.13, 8),
    "C2": (lambda: c2_args(48, 4), 0.13, 12),
    "partial": (lambda: ["-c", str(SCENES / "cornell_box.ecs"), "-size", "40", "24", "-spp", "4"], 0.13, 8),
    "dof": (SEQUENCES["dof"][0], 0.018, 8),
    "motion": (SEQUENCES["motion"][0], 0.23, 8),
}
# C1's outcome by the float64 formula on the oracle's sums: tiles stopped after each check
C1_STOPPED = {2: 6, 4: 7, 6: 9, 8: 10}


class Adaptive(Progressive):
    def adaptive(self, threshold, max_iterations, framebuffer=None, **kw):
        """(frame, stats, iterations per tile, error per tile) of one adaptive render."""
        fb = framebuffer or self.i["framebuffer"]
        st = self.dev.rtRenderAdaptive(self.i["renderer"], self.cam, self.i["scene"], self.i["tonemapper"], fb,
                                       threshold=threshold, max_iterations=max_iterations, **kw)
        it, err = self.dev.adaptive_tiles(fb)
        return self.dev.framebuffer_array(fb, self.W, self.H, self.fmt), st, it, err


_runs: dict = {}


def _run(dev, name, fmt="RGB_FLOAT32"):
    """The case's adaptive render, made once per format. Shared: do not modify."""
    if (name, fmt) not in _runs:
        args, thr, cap = CASES[name]
        p = Adaptive(dev, args(), fmt=fmt)
        img, st, it, err = p.adaptive(thr, cap)
        for a in (img, it, err):
            a.setflags(write=False)
        _runs[(name, fmt)] = dict(img=img, st=st, it=it, err=err, blob=p.blob, W=p.W, H=p.H, gamma=p.gamma)
        p.close()
    return _runs[(name, fmt)]


def _checks(cap):
    return range(2, cap + 1, 2)


def _restated(r, n):
    """E_T per tile (flat) at the check after n iterations, by the numpy restatement."""
    return tile_error(*sums_after(r["blob"], r["W"], r["H"], n)).reshape(-1)


def _last_check(n):
    return n - (n & 1)


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernel_is_the_header(gpu_device, name):
    """Every tile's reported error is yrt.tile_error (the header on the host) of the oracle-built
    sums after the tile's own iteration count, bit for bit."""
    r = _run(gpu_device, name)
    _, thr, cap = CASES[name]
    assert r["it"].size == ((r["W"] + 15) // 16) * ((r["H"] + 15) // 16) == r["st"]["tiles"]
    assert ((r["it"] >= 2) & (r["it"] <= cap) & (r["it"] % 2 == 0)).all(), r["it"]
    for n in sorted(set(r["it"].tolist())):
        want = yrt.tile_error(*sums_after(r["blob"], r["W"], r["H"], _last_check(n))).reshape(-1)
        sel = r["it"] == n
        assert np.array_equal(r["err"][sel].view(np.uint32), want[sel].view(np.uint32)), (name, n, r["err"], want)


@pytest.mark.parametrize("name", list(CASES))
def test_decisions_follow_the_errors(gpu_device, name):
    """A tile with count n below the cap reported E < threshold at n and, by the restatement, had
    E >= threshold at every earlier check; a tile at the cap never had E < threshold before the cap.
    All comparisons in float32 against the float32 threshold, as the kernel's."""
    r = _run(gpu_device, name)
    _, thr, cap = CASES[name]
    thr = np.float32(thr)
    E = {n: _restated(r, n) for n in _checks(cap)}
    closest = 1.0
    for t, n in enumerate(r["it"].tolist()):
        if n < cap:
            assert r["err"][t] < thr, (name, t, n, r["err"][t])
        for m in _checks(n):
            closest = min(closest, abs(float(E[m][t]) - float(thr)) / float(thr))
            if m < n:
                assert not (E[m][t] < thr), (name, t, n, m, E[m][t])
    print(f"{name}: counts {r['it'].tolist()}, closest error to the threshold {100 * closest:.2f} %")
    assert closest > 0.01, "a decision within 1 % of the threshold: pick the next threshold with clear gaps"
    stopped = int(sum(1 for t, n in enumerate(r["it"].tolist()) if r["err"][t] < thr))
    assert r["st"]["tilesStopped"] == stopped
    assert r["st"]["iterations"] == int(r["it"].max())
    below = {n for n in r["it"].tolist() if n < cap}
    assert len(below) >= 2 and (r["it"] == cap).any(), "everything or nothing stopped: the case shows little"
    if name == "C1":
        for n, count in C1_STOPPED.items():
            assert int(((r["it"] <= n) & (r["err"] < thr)).sum()) == count, (n, r["it"], r["err"])
    inside = np.minimum(16, r["W"] - 16 * (np.arange(r["it"].size) % ((r["W"] + 15) // 16))) * \
        np.minimum(16, r["H"] - 16 * (np.arange(r["it"].size) // ((r["W"] + 15) // 16)))
    assert r["st"]["samples"] == float((inside * r["it"]).sum() * 4)


@pytest.mark.parametrize("fmt", ["RGB_FLOAT32", "RGB8"])
@pytest.mark.parametrize("name", list(CASES))
def test_stopped_tiles_are_exact_prefixes(gpu_device, name, fmt):
    """Every tile with count n equals the plain progressive sequence after n calls on its pixels."""
    r = _run(gpu_device, name, fmt)
    f = _run(gpu_device, name)
    assert np.array_equal(r["it"], f["it"]) and np.array_equal(r["err"].view(np.uint32), f["err"].view(np.uint32))
    seq = oracle_sequence(r["blob"], r["W"], r["H"], r["gamma"], int(r["it"].max()))
    tx = (r["W"] + 15) // 16
    for t, n in enumerate(r["it"].tolist()):
        ys, xs = slice(16 * (t // tx), 16 * (t // tx) + 16), slice(16 * (t % tx), 16 * (t % tx) + 16)
        got, ref = r["img"][ys, xs], seq[n - 1][ys, xs]
        if fmt == "RGB8":
            ref8 = np.clip(ref * 255.0, 0, 255).astype(np.int32)
            assert np.array_equal(got.astype(np.int32), ref8), (name, t, n)
        else:
            _same(got, ref, f"{name} tile {t} after {n} iterations")
    assert len({n for n in r["it"].tolist()}) >= 2


def test_threshold_zero_is_the_progressive_sequence(gpu_device):
    """threshold = 0, maxIterations = 5: five rtRenderFrame(..., 1) calls, bit for bit; every tile
    ran 5 iterations (the checks after 2 and 4 ran and stopped nothing)."""
    p = Adaptive(gpu_device, c1_args(64, 4))
    img, st, it, err = p.adaptive(0.0, 5)
    assert (it == 5).all() and st["iterations"] == 5 and st["tilesStopped"] == 0 and st["tiles"] == 16
    assert st["samples"] == 64 * 64 * 4 * 5
    want = yrt.tile_error(*sums_after(p.blob, 64, 64, 4)).reshape(-1)
    assert np.array_equal(err.view(np.uint32), want.view(np.uint32))
    _same(img, p.oracle(5)[4], "threshold 0 after 5 iterations")
    plain = [p.frame(1 if k else 0) for k in range(5)][4]
    assert np.array_equal(img, plain)
    img1, st1, it1, err1 = p.adaptive(-1.0, 1)  # an odd cap below the first check
    assert (it1 == 1).all() and np.isposinf(err1).all() and st1["iterations"] == 1
    _same(img1, p.oracle(1)[0], "one iteration")
    p.close()


def test_list_mode_does_not_depend_on_batching(gpu_device):
    """The same adaptive render with 1, 3 and all active tiles in a batch, on 1 and 3 lanes."""
    dev = gpu_device
    r = _run(dev, "C1")
    args, thr, cap = CASES["C1"]
    p = Adaptive(dev, args())
    try:
        for lanes, capacity in ((1, 1024), (1, 3072), (1, 64 << 20), (3, 1024), (3, 3072), (3, 64 << 20)):
            dev.set_lanes(lanes)
            dev.set_batch_capacity(capacity)  # 4 spp: 1024 paths a tile
            img, st, it, err = p.adaptive(thr, cap)
            what = f"{lanes} lanes, {capacity} paths"
            assert np.array_equal(it, r["it"]) and np.array_equal(err.view(np.uint32), r["err"].view(np.uint32)), what
            assert np.array_equal(img, r["img"]), what
            assert st["samples"] == r["st"]["samples"]
    finally:
        dev.set_lanes(0)
        dev.set_batch_capacity(64 << 20)
        p.close()


def test_state_afterwards(gpu_device):
    """accumulate=1 after an adaptive render is refused until accumulate=0 restarts the plain
    sequence; the renderer's iteration is n; a second framebuffer refined in between is untouched; a
    device of two render contexts refuses the call."""
    dev = gpu_device
    args, thr, cap = CASES["C1"]
    a, b = Adaptive(dev, args()), Progressive(dev, c2_args(64, 4))
    try:
        ra, rb = a.oracle(2), b.oracle(3)
        for k in range(2):
            _same(b.frame(1 if k else 0), rb[k], f"B call {k}")
        img, st, it, err = a.adaptive(thr, cap)
        assert np.array_equal(img, _run(dev, "C1")["img"])
        _same(b.frame(1), rb[2], "B call 2, after A's adaptive render")
        with pytest.raises(RuntimeError, match="adaptive render"):
            a.frame(1)
        assert np.array_equal(dev.adaptive_tiles(a.i["framebuffer"])[0], it)  # the refusal changed nothing
        _same(a.frame(0), ra[0], "accumulate=0 after the adaptive render")
        _same(a.frame(1), ra[1], "accumulate=1 after the restart")
        img2 = a.adaptive(thr, cap)[0]
        assert np.array_equal(img2, img), "a second adaptive render into the same framebuffer"
    finally:
        a.close()
        b.close()
    two = yrt.Device(devices=[0, 0])
    try:
        p = Adaptive(two, args())
        with pytest.raises(RuntimeError, match="render contexts"):
            p.adaptive(thr, cap)
        _same(p.frame(0), p.oracle(1)[0], "the refusal changed nothing")
        p.close()
    finally:
        two.close()


def test_front_end(gpu_device):
    """-adaptive <threshold> <maxIterations>: `-adaptive 0 3` on C1 is the third progressive frame,
    `-adaptive 0.13 8` the adaptive frame of the API call."""
    r = _run(gpu_device, "C1")
    s = yrt.Session(c1_args(64, 4) + ["-fb", "RGB_FLOAT32", "-adaptive", "0", "3"], device=gpu_device)
    img = s.render()
    _same(img, oracle_sequence(s.export_frame(), 64, 64, s.info()["gamma"], 3)[2], "-adaptive 0 3")
    s.close()
    s = yrt.Session(c1_args(64, 4) + ["-fb", "RGB_FLOAT32", "-adaptive", "0.13", "8"], device=gpu_device)
    img = s.render()
    it, err = gpu_device.adaptive_tiles(s.info()["framebuffer"])
    s.close()
    assert np.array_equal(it, r["it"]) and np.array_equal(img, r["img"])
