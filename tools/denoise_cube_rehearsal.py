#!/usr/bin/env python3
"""The cube denoise ("cube"): does filtering across the cube's edges remove the seam?

The Cornell box seen from inside (eye (278, 273, 250), looking 25 degrees off +z, up (0, 1, 0),
-stereo), left eye, gamma 2.2, 4 spp against a converged frame, default weights. Over the hit
pixels below 1 in both frames:
  seam error   for every pixel p of a face's last column and the pixel q the tap one step to its
               right lands on: mean |(c(p) - c(q)) - (conv(p) - conv(q))|
  band mse     mean squared error against the converged frame over the b-pixel border band
for the raw frame, the per-face filter and the cube filter.

  default  CPU rehearsal: the oracle's frames, guides from the oracle's camera rays (pixel centres,
           geometric normals), the numpy filters of tests/denoise_ref.py and tests/denoise_cube_ref.py.
  --gpu    the device's frames, guides and filters (yrtDenoiseFrameBuffer per face, yrtDenoiseCube).
  --cost   yrtGetDenoiseTimes of yrtDenoiseCube against the loop of per-face calls on the C4 cube
           map (12 faces of --big^2, frames in HBM), RGB8 and RGB_FLOAT32, plain and demodulated,
           three repetitions each.

usage: python tools/denoise_cube_rehearsal.py [--gpu] [--cost] [--size 64] [--spp 1024] [--iterations 5] [--big 1536]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "yulio-raytracer_amd"), str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

import yrt  # noqa: E402

import denoise_cube_ref as cref  # noqa: E402
import denoise_ref as ref  # noqa: E402

WEIGHTS = dict(sigma_color=1.0, sigma_normal=64.0, sigma_position=float(np.float32(0.02)))
POWER = 1 / 2.2


def measures(frames, conv, ok, bands=(1, 2, 4)):
    """frames: {name: (6, W, W, 3)}; ok (6, W, W): the pixels that count."""
    return {name: (cref.seam_error(c, conv, ok), [cref.band_mse(c, conv, ok, b) for b in bands])
            for name, c in frames.items()}


def report(title, m, bands=(1, 2, 4)):
    print(title)
    for name, (seam, mse) in m.items():
        print(f"  {name:9s} seam error {seam:.6g}   band mse " +
              "  ".join(f"{b} px {v:.6g}" for b, v in zip(bands, mse)))
    s0, s1 = m["per-face"][0], m["cube"][0]
    print(f"  cube / per-face: seam {s1 / s0:.4f}   band mse " +
          "  ".join(f"{b} px {c / p:.4f}" for b, p, c in zip(bands, m["per-face"][1], m["cube"][1])))


def cpu(args):
    import oracle
    W = args.size
    dev = yrt.Device(host=True)
    frames = []
    blobs = None
    for spp in (4, args.spp):
        s = yrt.Session(cref.cube_args(W, spp), device=dev)
        blobs = [s.export_frame(f) for f in range(6)]
        gamma = s.info()["gamma"]
        frames.append(np.stack([oracle.render(b, W, W, gamma)[0].astype(np.float64) for b in blobs]))
        s.close()
    raw, conv = frames
    c = (np.arange(W, dtype=np.float32) + np.float32(0.5)) / np.float32(W)
    px = np.stack(np.meshgrid(c, c), -1).reshape(-1, 2)
    tris = oracle.scene_triangles(blobs[0]).astype(np.float64)
    pos4 = np.zeros((6, W * W, 4), np.float32)
    nrm4 = np.zeros((6, W * W, 4), np.float32)
    for f, blob in enumerate(blobs):
        org, dr = oracle.camera_rays(blob, px)
        n = len(px)
        hit = oracle.trace(blob, np.concatenate([org, np.zeros((n, 1), np.float32)], 1),
                           np.concatenate([dr, np.full((n, 1), np.inf, np.float32)], 1))
        tri = hit[:, 3].copy().view(np.int32)
        ok = tri >= 0
        pos4[f, :, 3] = np.inf
        pos4[f, ok, :3] = org[ok] + hit[ok, :1] * dr[ok]
        pos4[f, ok, 3] = hit[ok, 0]
        t9 = tris[tri[ok]]
        ng = np.cross(t9[:, 0:3] - t9[:, 3:6], t9[:, 6:9] - t9[:, 0:3])
        ng /= np.linalg.norm(ng, axis=1, keepdims=True)
        ng[(ng * dr[ok]).sum(1) > 0] *= -1
        nrm4[f, ok, :3] = ng
        nrm4[f, ok, 3] = 1
    pos4, nrm4 = pos4.reshape(6, W, W, 4), nrm4.reshape(6, W, W, 4)
    per_face = np.stack([ref.atrous(raw[f], pos4[f], nrm4[f], args.iterations, **WEIGHTS) for f in range(6)])
    cube = cref.atrous_cube(raw, pos4, nrm4, args.iterations, **WEIGHTS)
    ok = np.isfinite(pos4[..., 3]) & (conv.max(-1) < 1) & (raw.max(-1) < 1)
    R = 2 * (2 ** args.iterations - 1)
    if W > 2 * R:
        print(f"interior (at least {R} from every border) equal between the two filters: "
              f"{np.array_equal(per_face[:, R:W - R, R:W - R], cube[:, R:W - R, R:W - R])}")
    report(f"CPU rehearsal: oracle frames, numpy filters; {W} x {W} faces, 4 spp against {args.spp} spp, "
           f"{args.iterations} iterations; {ok.mean():.4f} of the pixels count",
           measures({"raw": raw, "per-face": per_face, "cube": cube}, conv, ok))


def gpu_frames(d, W, spp, iterations):
    """(raw, per-face filtered, cube filtered, hit mask) of the left eye on the device, float64."""
    s = yrt.Session(cref.cube_args(W, spp) + ["-fb", "RGB_FLOAT32"], device=d)
    i = s.info()
    cams = [s.camera(f) for f in range(6)]

    def job():
        fbs = [d.rtNewFrameBuffer("RGB_FLOAT32", W, W) for _ in cams]
        d.rtRenderFrames(i["renderer"], cams, i["scene"], i["tonemapper"], fbs, 0)
        return fbs

    def read(fbs):
        return np.stack([d.framebuffer_array(fb, W, W, "RGB_FLOAT32") for fb in fbs]).astype(np.float64)

    raw = read(job())
    out = [raw]
    if iterations:
        fbs = job()
        for cam, fb in zip(cams, fbs):
            d.denoise(cam, i["scene"], fb, iterations=iterations)
        out.append(read(fbs))
        fbs = job()
        d.denoise_cube(cams, i["scene"], fbs, iterations=iterations)
        out.append(read(fbs))
        out.append(np.stack([np.isfinite(d.render_guides(cam, i["scene"], W, W)[0][..., 3]) for cam in cams]))
    s.close()
    return out


def gpu(args):
    W = args.size
    d = yrt.Device(0)
    conv = gpu_frames(d, W, args.spp, 0)[0]
    raw, per_face, cube, hit = gpu_frames(d, W, 4, args.iterations)
    ok = hit & (conv.max(-1) < 1) & (raw.max(-1) < 1)
    report(f"MI355X: the device's frames and filters; {W} x {W} faces, 4 spp against {args.spp} spp, "
           f"{args.iterations} iterations; {ok.mean():.4f} of the pixels count",
           measures({"raw": raw, "per-face": per_face, "cube": cube}, conv, ok))


def cost(args):
    from helpers import c4_args
    B = args.big
    d = yrt.Device(0)
    d.set_kernel_timing(True)
    for fmt in ("RGB8", "RGB_FLOAT32"):
        s = yrt.Session(c4_args(B, 1) + ["-fb", fmt, "-gamma", "2.2"], device=d)
        i = s.info()
        cams = [s.camera(f) for f in range(12)]
        fbs = [d.rtNewFrameBuffer(fmt, B, B) for _ in cams]
        for rep in range(3):
            for name, kw in (("plain", {}), ("demodulated", dict(demodulate=1, albedo_power=POWER))):
                d.rtRenderFrames(i["renderer"], cams, i["scene"], i["tonemapper"], fbs, 0)
                g = f = 0.0
                for cam, fb in zip(cams, fbs):
                    d.denoise(cam, i["scene"], fb, **kw)
                    a, b = d.denoise_times()
                    g, f = g + a, f + b
                print(f"{fmt:12s} 12 x {B}^2 in HBM  rep {rep}: {name:12s} loop of 12  guides {g:8.3f} ms   "
                      f"filter x5 {f:8.3f} ms", flush=True)
                d.rtRenderFrames(i["renderer"], cams, i["scene"], i["tonemapper"], fbs, 0)
                d.denoise_cube(cams, i["scene"], fbs, **kw)
                g, f = d.denoise_times()
                print(f"{fmt:12s} 12 x {B}^2 in HBM  rep {rep}: {name:12s} cube call   guides {g:8.3f} ms   "
                      f"filter x5 {f:8.3f} ms", flush=True)
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--big", type=int, default=1536)
    args = ap.parse_args()
    if args.cost:
        cost(args)
    else:
        (gpu if args.gpu else cpu)(args)


if __name__ == "__main__":
    main()
