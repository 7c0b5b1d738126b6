"""Adaptive sampling on C3 (Sponza stand-in, 2048^2, 8 spp an iteration), the record in
profiles/adaptive_c3.txt: the loop's cost with nothing stopping (threshold 0 against the same
number of accumulate=1 calls), and time, samples, tiles per stop count and RMSE against a 1024-spp
frame over a few thresholds and iteration caps, beside plain frames of the same sample counts.

    python tools/adaptive_c3.py > profiles/adaptive_c3.txt    (one MI355X; about a minute)
"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "yulio-raytracer_amd"), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import yrt  # noqa: E402
from helpers import c3_args  # noqa: E402


def say(*a):
    print(*a, flush=True)


SIZE, SPP, ITER = 2048, 8, 8
dev = yrt.Device(0)
ses = yrt.Session(c3_args(SIZE, SPP) + ["-fb", "RGB_FLOAT32"], device=dev)
i = ses.info()
cam = ses.camera()
fb = i["framebuffer"]


def frame():
    return dev.framebuffer_array(fb, SIZE, SIZE, "RGB_FLOAT32")


def plain(n):
    t = time.perf_counter()
    for k in range(n):
        dev.rtRenderFrame(i["renderer"], cam, i["scene"], i["tonemapper"], fb, 1 if k else 0)
    dev.rtMapFrameBuffer(fb)
    dev.rtUnmapFrameBuffer(fb)
    return (time.perf_counter() - t) * 1e3


def adaptive(thr, cap):
    t = time.perf_counter()
    st = dev.rtRenderAdaptive(i["renderer"], cam, i["scene"], i["tonemapper"], fb, threshold=thr, max_iterations=cap)
    dev.rtMapFrameBuffer(fb)
    dev.rtUnmapFrameBuffer(fb)
    return (time.perf_counter() - t) * 1e3, st


plain(2)
adaptive(0.0, 2)  # warm up: sample tables of the first iterations, buffers
say(f"# C3 stand-in {SIZE}^2, {SPP} spp an iteration, gamma {i['gamma']}, wall-clock ms incl. the frame's read-back")
say("## 2. the loop with nothing stopping: threshold 0, 8 iterations, against eight accumulate=1 calls")
tp, ta, te = [], [], []
for r in range(5):
    tp.append(plain(ITER))
    ms, st = adaptive(0.0, ITER)
    ta.append(ms)
    te.append(st["msError"])
    say(f"run {r}: plain x8 {tp[-1]:.1f} ms   adaptive(0, 8) {ta[-1]:.1f} ms (checks {te[-1]:.2f} ms, tiles stopped {st['tilesStopped']})")
mp, ma = statistics.median(tp), statistics.median(ta)
say(f"median: plain {mp:.1f} ms, adaptive {ma:.1f} ms, overhead {ma - mp:+.1f} ms ({100 * (ma / mp - 1):+.2f} %), "
    f"of which the 4 checks {statistics.median(te):.2f} ms")
a0 = frame()
plain(ITER)
assert np.array_equal(a0, frame()), "threshold 0 differs from the plain sequence"
say("threshold 0 frame == the eighth plain progressive frame, bit for bit")

say("## 3. thresholds")
ref_ses = yrt.Session(c3_args(SIZE, 1024) + ["-fb", "RGB_FLOAT32"], device=dev)
t = time.perf_counter()
ref = ref_ses.render().astype(np.float64)
say(f"reference: one 1024-spp frame, {(time.perf_counter() - t) * 1e3:.0f} ms")
ref_ses.close()


def rmse(img):
    return float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))


s64 = yrt.Session(c3_args(SIZE, 64) + ["-fb", "RGB_FLOAT32"], device=dev)
s64.render()
ts = []
for r in range(3):
    t = time.perf_counter()
    img64 = s64.render()
    ts.append((time.perf_counter() - t) * 1e3)
s64.close()
say(f"plain 64-spp frame (one call): {statistics.median(ts):.1f} ms, RMSE {rmse(img64):.5f}")
t8 = statistics.median([plain(ITER) for _ in range(3)])
say(f"plain 8 x 8 spp (accumulate=1): {t8:.1f} ms, RMSE {rmse(frame()):.5f}")
for n in (16, 32):
    tn = statistics.median([plain(n) for _ in range(3)])
    say(f"plain {n} x 8 spp (accumulate=1): {tn:.1f} ms, RMSE {rmse(frame()):.5f}")
for cap in (8, 16, 32):
    say(f"-- maxIterations {cap}")
    for thr in (0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2):
        ms = []
        for r in range(3):
            m, st = adaptive(thr, cap)
            ms.append(m)
        it, err = dev.adaptive_tiles(fb)
        hist = {int(n): int((it == n).sum()) for n in sorted(set(it.tolist()))}
        say(f"threshold {thr:<7} {statistics.median(ms):7.1f} ms  samples {st['samples'] / 1e6:7.1f} M "
            f"({st['samples'] / (SIZE * SIZE):5.1f} spp mean)  stopped {st['tilesStopped']:5d}/{st['tiles']}  "
            f"RMSE {rmse(frame()):.5f}  checks {st['msError']:.2f} ms  tiles per count {hist}")
fin = err[np.isfinite(err)]
say(f"last errors at threshold 0.2, cap 32: min {fin.min():.4f} median {np.median(fin):.4f} max {fin.max():.4f}")
ses.close()
dev.close()
