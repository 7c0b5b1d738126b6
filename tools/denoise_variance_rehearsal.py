#!/usr/bin/env python3
"""The variance-guided denoise path at 64 x 64: mean squared error against the
1024-spp frame of the plain filter (sigmaColor 0.25, 0.5, 1, 2) and of the variance-guided filter
(sigmaVariance 1, 2, 3, 4, varianceFloor (1/255)^2), over the raw frame's, for C1 and C2 rendered as
2 and as 8 progressive iterations of 4 spp; whole frame and the pixels below 1 in both frames.

  default  CPU rehearsal: the oracle's iteration sums (tests/adaptive_ref.py), guides from the
           oracle's camera rays (pixel centres, geometric normals), the variance frame by the
           shared header on the host (yrt.frame_variance), the numpy filters of tests/denoise_ref.py
           and tests/denoise_variance_ref.py.
  --gpu    the device's frames (rtRenderAdaptive, threshold 0), variance frame and filters; and,
           unless --no-times, yrtGetDenoiseTimes at --big^2 (default 2048) on C3 after
           rtRenderAdaptive(threshold 0, 2 iterations of 4 spp), plain against variance-guided.

The default sigmaVariance is the candidate with the lowest sum of the four below-1 ratios of the CPU
rehearsal; the tool prints it.

usage: python tools/denoise_variance_rehearsal.py [--gpu] [--size 64] [--big 2048] [--no-times]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "yulio-raytracer_amd"), str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

import yrt  # noqa: E402

import denoise_ref as ref  # noqa: E402
import denoise_variance_ref as vref  # noqa: E402
from helpers import c1_args, c2_args  # noqa: E402

SIGMA_COLORS = (0.25, 0.5, 1.0, 2.0)
SIGMA_VARIANCES = (1.0, 2.0, 3.0, 4.0)
WEIGHTS = dict(sigma_normal=64.0, sigma_position=float(np.float32(0.02)))
SPP, CONVERGED, FILTER_ITERATIONS = 4, 1024, 5
SCENES = {"C1": c1_args, "C2": c2_args}
CASES = [("C1", 2), ("C2", 2), ("C1", 8), ("C2", 8)]


def oracle_guides(blob, size):
    """(pos4, nrm4), (size, size, 4) float32: the first hits of the oracle's camera rays through the
    pixel centres as (point, t) and (geometric normal towards the viewer, 1); a miss (0, 0, 0, inf), 0."""
    import oracle
    c = (np.arange(size, dtype=np.float32) + np.float32(0.5)) / np.float32(size)
    px = np.stack(np.meshgrid(c, c), -1).reshape(-1, 2)
    org, dr = oracle.camera_rays(blob, px)
    n = len(px)
    org4 = np.concatenate([org, np.zeros((n, 1), np.float32)], 1)
    dir4 = np.concatenate([dr, np.full((n, 1), np.inf, np.float32)], 1)
    hit = oracle.trace(blob, org4, dir4)
    tri = hit[:, 3].copy().view(np.int32)
    ok = tri >= 0
    tris = oracle.scene_triangles(blob).astype(np.float64)
    pos4 = np.zeros((n, 4), np.float32)
    pos4[:, 3] = np.inf
    nrm4 = np.zeros((n, 4), np.float32)
    pos4[ok, :3] = org[ok] + hit[ok, :1] * dr[ok]
    pos4[ok, 3] = hit[ok, 0]
    t9 = tris[tri[ok]]
    ng = np.cross(t9[:, 0:3] - t9[:, 3:6], t9[:, 6:9] - t9[:, 0:3])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    ng[(ng * dr[ok]).sum(1) > 0] *= -1
    nrm4[ok, :3] = ng
    nrm4[ok, 3] = 1
    return pos4.reshape(size, size, 4), nrm4.reshape(size, size, 4)


_inputs: dict = {}


def oracle_inputs(scene, size, iterations):
    """dict(raw, conv, var4, pos4, nrm4) of `scene` after `iterations` progressive iterations of SPP
    samples: raw the displayed running mean, conv the CONVERGED-spp frame. Shared: do not modify."""
    import oracle
    from adaptive_ref import sums_after
    key = (scene, size)
    if key not in _inputs:
        dev = yrt.Device(host=True)
        s = yrt.Session(SCENES[scene](size, SPP), device=dev)
        blob, gamma = s.export_frame(), float(s.info()["gamma"])
        s.close()
        s = yrt.Session(SCENES[scene](size, CONVERGED), device=dev)
        conv = oracle.render(s.export_frame(), size, size, gamma)[0].astype(np.float64)
        s.close()
        dev.close()
        _inputs[key] = (blob, gamma, conv) + oracle_guides(blob, size)
    blob, gamma, conv, pos4, nrm4 = _inputs[key]
    accu, half = sums_after(blob, size, size, iterations)
    mean = accu[..., :3].astype(np.float64) / accu[..., 3:4]
    raw = mean ** (1.0 / gamma) if gamma != 1.0 else mean
    return dict(raw=raw, conv=conv, var4=yrt.frame_variance(accu, half, gamma), pos4=pos4, nrm4=nrm4)


def cpu_filters(scene, size, iterations):
    """(raw, conv, plain(sigmaColor) -> frame, guided(sigmaVariance) -> frame) on the oracle's inputs."""
    d = oracle_inputs(scene, size, iterations)

    def plain(sc):
        return ref.atrous(d["raw"], d["pos4"], d["nrm4"], FILTER_ITERATIONS, sigma_color=sc, **WEIGHTS)

    def guided(k):
        return vref.atrous_var(d["raw"], d["var4"], d["pos4"], d["nrm4"], FILTER_ITERATIONS, k, vref.FLOOR, **WEIGHTS)

    return d["raw"], d["conv"], plain, guided


def gpu_filters(dev, scene, size, iterations):
    s = yrt.Session(SCENES[scene](size, CONVERGED) + ["-fb", "RGB_FLOAT32"], device=dev)
    conv = s.render().astype(np.float64)
    s.close()
    s = yrt.Session(SCENES[scene](size, SPP) + ["-fb", "RGB_FLOAT32"], device=dev)
    i = s.info()

    def frame(**kw):
        dev.rtRenderAdaptive(i["renderer"], s.camera(), i["scene"], i["tonemapper"], i["framebuffer"], threshold=0.0,
                             max_iterations=iterations)
        if kw:
            dev.denoise(s.camera(), i["scene"], i["framebuffer"], iterations=FILTER_ITERATIONS, **kw)
        return dev.framebuffer_array(i["framebuffer"], size, size, "RGB_FLOAT32").astype(np.float64)

    raw = frame()
    return raw, conv, (lambda sc: frame(sigma_color=sc)), (lambda k: frame(variance_guided=1, sigma_variance=k)), s


def table(filters):
    """Prints the rows; returns {sigmaVariance: sum of the below-1 ratios}."""
    sums = {k: 0.0 for k in SIGMA_VARIANCES}
    print("values: MSE against the %d-spp frame over the raw frame's; (whole frame / pixels below 1)" % CONVERGED)
    print("case               " + "".join(f"plain sc={sc:<12g}" for sc in SIGMA_COLORS) +
          "".join(f"guided k={k:<11g}" for k in SIGMA_VARIANCES))
    for scene, n in CASES:
        raw, conv, plain, guided = filters(scene, n)[:4]
        row = f"{scene}, {n} iterations   "
        for sc in SIGMA_COLORS:
            w, b = vref.mse_ratios(plain(sc), raw, conv)
            row += f"{w:7.4f} / {b:7.4f}   "
        for k in SIGMA_VARIANCES:
            w, b = vref.mse_ratios(guided(k), raw, conv)
            sums[k] += b
            row += f"{w:7.4f} / {b:7.4f}   "
        print(row, flush=True)
    print("sum of the four below-1 ratios per sigmaVariance: " + ", ".join(f"{k:g}: {v:.4f}" for k, v in sums.items()))
    print(f"lowest: sigmaVariance {min(sums, key=sums.get):g}")
    return sums


def cpu(args):
    print(f"CPU rehearsal: oracle sums, numpy filters; {args.size} x {args.size}, {SPP} spp per iteration, "
          f"{FILTER_ITERATIONS} filter iterations, varianceFloor (1/255)^2")
    return table(lambda scene, n: cpu_filters(scene, args.size, n))


def times(dev, big):
    from yrt import standin
    dev.set_kernel_timing(True)
    c3 = ["-i", str(standin.write_xml())] + standin.C3_ARGS + ["-size", str(big), str(big), "-spp", str(SPP)]
    for fmt in ("RGB8", "RGB_FLOAT32"):
        s = yrt.Session(c3 + ["-fb", fmt], device=dev)
        i = s.info()
        for rep in range(3):
            for name, kw in (("plain", {}), ("variance-guided", dict(variance_guided=1))):
                st = dev.rtRenderAdaptive(i["renderer"], s.camera(), i["scene"], i["tonemapper"], i["framebuffer"],
                                          threshold=0.0, max_iterations=2)
                dev.denoise(s.camera(), i["scene"], i["framebuffer"], **kw)
                g, f = dev.denoise_times()
                print(f"{fmt:12s} {big} x {big} frame in HBM  rep {rep}: {name:16s} render (2 x {SPP} spp) "
                      f"{st['msTotal']:9.3f} ms   guides {g:7.3f} ms   filter x5 {f:7.3f} ms   "
                      f"filter / render {f / st['msTotal']:.4f}", flush=True)
        s.close()


def gpu(args):
    dev = yrt.Device(0)
    print(f"MI355X: the device's frames, variance frame and filters; {args.size} x {args.size}, {SPP} spp per "
          f"iteration, {FILTER_ITERATIONS} filter iterations, varianceFloor (1/255)^2")
    open_sessions = []

    def filters(scene, n):
        r = gpu_filters(dev, scene, args.size, n)
        for s in open_sessions:
            s.close()
        open_sessions[:] = [r[4]]
        return r

    table(filters)
    for s in open_sessions:
        s.close()
    if not args.no_times:
        times(dev, args.big)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--no-times", action="store_true")
    args = ap.parse_args()
    (gpu if args.gpu else cpu)(args)


if __name__ == "__main__":
    main()
