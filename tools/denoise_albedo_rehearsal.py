#!/usr/bin/env python3
"""The texture-preserving denoise path at 64 x 64,
gamma 2.2, 4 spp against 1024 spp: mean squared error of the raw, the plain-filtered and the
demodulated frame of a textured scene over the pixels below 1 in both frames, for sigmaColor 0.25, 0.5, 1 and 2.

  default  CPU rehearsal: the oracle's frames, guides from the oracle's camera rays (pixel centres,
           geometric normals), the albedo restated in numpy from the scene's meshes and images
           (bilinear Kd lookup, or the stand-in cloth's diffuse colour), the numpy filters of
           tests/denoise_ref.py and tests/denoise_albedo_ref.py.
  --gpu    the device's frames, guides, albedo and filter; also the numpy albedo against
           yrtRenderAlbedo, and yrtGetDenoiseTimes at --big^2 (default 2048) on C3 with and without
           demodulation.

Scenes: `room` (tests/denoise_albedo_ref.py: the Cornell box with MatteTextured walls and a block,
the scene of tests/test_denoise_albedo.py) and `c3` (the Sponza stand-in under a dome of --dome).

usage: python tools/denoise_albedo_rehearsal.py [--gpu] [--scene room|c3] [--size 64] [--big 2048] [--dome 1]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "yulio-raytracer_amd"), str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

import yrt  # noqa: E402
from yrt import standin  # noqa: E402

import denoise_albedo_ref as aref  # noqa: E402
import denoise_ref as ref  # noqa: E402

SIGMAS = (0.25, 0.5, 1.0, 2.0)
WEIGHTS = dict(sigma_normal=64.0, sigma_position=float(np.float32(0.02)))
POWER, FLOOR = 1 / 2.2, float(np.float32(1 / 255))


def c3_dim_args(size, spp, dome):
    """C3's scene and camera (the textured Sponza stand-in) under a dome of radiance `dome` instead of
    8: with 1 every surface pixel of the gamma-2.2 frame stays below 1."""
    x = standin.write_xml()
    a = ["-i", str(x)] + standin.C3_ARGS + ["-size", str(size), str(size), "-spp", str(spp)]
    i = a.index("-ambientlight")
    a[i + 1:i + 4] = [str(dome)] * 3
    return a + ["-fb", "RGB_FLOAT32", "-gamma", "2.2"]


def scene_c3(args):
    """(session arguments for size and spp, [(texcoords, triangles, image (H, W, 3) float32 or colour)])"""
    meshes = []
    for m in standin.build_meshes():
        _, _, T, I = m.arrays()
        tex, colour = m.material
        img = colour
        if tex:  # the JPEG loader stores the rows bottom-up
            img = yrt.decode_image(standin.SCENES / "Sponza" / tex)[::-1, :, :3].astype(np.float32) / np.float32(255)
        meshes.append((T, I, img))
    return (lambda size, spp: c3_dim_args(size, spp, args.dome)), meshes


def scene_room(args):
    xml = aref.write_room(ROOT / "scenes" / "_generated")
    tex = [t.astype(np.float32) / np.float32(255) for t in aref.room_textures()]
    meshes = [(aref.QUAD_ST, aref.QUAD_IDX, tex[k]) for _, k in aref.room_quads()]
    return (lambda size, spp: aref.room_args(xml, size, spp)), meshes


def numpy_albedo(hit, meshes):
    """(n, 4) albedo of oracle.trace hits (t, u, v, triangle id bits); the triangle ids count through
    `meshes` in order. Uber / MatteTextured with s0 = 0, ds = 1: the bilinear Kd lookup, or the colour."""
    tri = hit[:, 3].copy().view(np.int32)
    u, v = hit[:, 1].astype(np.float64), hit[:, 2].astype(np.float64)
    out = np.zeros((len(hit), 4), np.float32)
    first = 0
    for T, I, img in meshes:
        sel = (tri >= first) & (tri < first + len(I))
        if sel.any():
            if np.ndim(img) == 3:
                st = T[I[tri[sel] - first]].astype(np.float64)           # (k, 3 vertices, 2)
                w = 1 - u[sel] - v[sel]
                s = st[:, 0, 0] * w + st[:, 1, 0] * u[sel] + st[:, 2, 0] * v[sel]
                t = st[:, 0, 1] * w + st[:, 1, 1] * u[sel] + st[:, 2, 1] * v[sel]
                out[sel, :3] = aref.lookup_bilinear(img, s, t)
            else:
                out[sel, :3] = img
            out[sel, 3] = 1
        first += len(I)
    out[tri >= first] = 1  # a light primitive's triangles come after the meshes'
    zero = (out[:, 3] == 1) & (out[:, :3] == 0).all(1)
    out[zero, :3] = 1
    return out, first


def oracle_inputs(size, scene):
    import oracle
    dev = yrt.Device(host=True)
    frames, blob = [], None
    for spp in (4, 1024):
        s = yrt.Session(scene[0](size, spp), device=dev)
        blob = s.export_frame()
        frames.append(oracle.render(blob, size, size, s.info()["gamma"])[0].astype(np.float64))
        s.close()
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
    alb = np.zeros((n, 4), np.float32)
    alb[ok], count = numpy_albedo(hit[ok], scene[1])
    assert count <= len(tris), (count, len(tris))  # the light primitives' triangles come after the meshes'
    shape = (size, size, 4)
    return frames[0], frames[1], pos4.reshape(shape), nrm4.reshape(shape), alb.reshape(shape), hit


def table(raw, conv, plain, demod):
    dark = (conv.max(-1) < 1) & (raw.max(-1) < 1)

    def mse(f):
        return float(((f - conv)[dark] ** 2).mean())

    print(f"pixels below 1 in both frames: {dark.mean():.4f} of the frame; mse raw {mse(raw):.6g}")
    print("sigmaColor   plain (/ raw)         demodulated (/ raw)   demodulated / plain")
    for sc in SIGMAS:
        p, d = mse(plain(sc)), mse(demod(sc))
        print(f"{sc:<10g}   {p:.6g} ({p / mse(raw):.4f})   {d:.6g} ({d / mse(raw):.4f})   {d / p:.4f}")


def cpu(args):
    raw, conv, pos4, nrm4, alb, _ = oracle_inputs(args.size, args.scene)
    print(f"CPU rehearsal: oracle frames, numpy filter; {args.name}, {args.size} x {args.size}, "
          f"gamma 2.2, 4 spp against 1024 spp, 5 iterations")
    table(raw, conv, lambda sc: ref.atrous(raw, pos4, nrm4, 5, sigma_color=sc, **WEIGHTS),
          lambda sc: aref.demodulated_atrous(raw, pos4, nrm4, alb, 5, POWER, FLOOR, sigma_color=sc, **WEIGHTS))


def gpu(args):
    S = args.size
    d = yrt.Device(0)
    s = yrt.Session(args.scene[0](S, 1024), device=d)
    conv = s.render().astype(np.float64)
    s.close()
    s = yrt.Session(args.scene[0](S, 4), device=d)
    raw = s.render().astype(np.float64)
    i = s.info()

    def filtered(**kw):
        s.render(read=False)
        d.denoise(s.camera(), i["scene"], i["framebuffer"], **kw)
        return d.framebuffer_array(i["framebuffer"], S, S, "RGB_FLOAT32").astype(np.float64)

    print(f"MI355X: the device's frames and filter; {args.name}, {S} x {S}, gamma 2.2, "
          f"4 spp against 1024 spp, 5 iterations")
    table(raw, conv, lambda sc: filtered(sigma_color=sc),
          lambda sc: filtered(sigma_color=sc, demodulate=1, albedo_power=POWER))
    alb = d.render_albedo(s.camera(), i["scene"], S, S)
    s.close()
    try:
        *_, want, hit = oracle_inputs(S, args.scene)
        both = (alb[..., 3] == 1) & (want[..., 3] == 1)
        err = np.abs(alb[both][:, :3].astype(np.float64) - want[both][:, :3])
        print(f"yrtRenderAlbedo against the numpy albedo of the rehearsal: hit masks equal "
              f"{np.array_equal(alb[..., 3], want[..., 3])}, max |difference| {err.max():.3g}, "
              f"{(err.max(1) > 1e-4).mean():.4f} of the hit pixels differ by more than 1e-4")
    except Exception as e:  # the oracle library may be absent
        print(f"numpy albedo comparison skipped: {e}")

    if args.no_times:
        return
    B = args.big
    d.set_kernel_timing(True)
    c3 = ["-i", str(standin.write_xml())] + standin.C3_ARGS + ["-size", str(B), str(B), "-spp", "4", "-gamma", "2.2"]
    for fmt in ("RGB8", "RGB_FLOAT32"):
        s = yrt.Session(c3 + ["-fb", fmt], device=d)
        i = s.info()
        for rep in range(3):
            for name, kw in (("plain", {}), ("demodulated", dict(demodulate=1, albedo_power=POWER))):
                s.render(read=False)
                d.denoise(s.camera(), i["scene"], i["framebuffer"], **kw)
                g, f = d.denoise_times()
                print(f"{fmt:12s} {B} x {B} frame in HBM  rep {rep}: {name:12s} guides {g:8.3f} ms   filter x5 {f:8.3f} ms")
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--dome", type=float, default=1.0, help="c3: the dome's radiance (C3 itself has 8)")
    ap.add_argument("--scene", choices=("room", "c3"), default="room")
    ap.add_argument("--no-times", action="store_true")
    args = ap.parse_args()
    args.name = "the textured room" if args.scene == "room" else f"Sponza stand-in, dome {args.dome:g}"
    args.scene = (scene_room if args.scene == "room" else scene_c3)(args)
    (gpu if args.gpu else cpu)(args)


if __name__ == "__main__":
    main()
