#!/usr/bin/env python3
"""sha256 of what the denoise stage gives on the GPU, to compare two builds of the library bit for bit.

The package and the test scenes are this tree's; YRT_LIB_DIR selects whose libraries run (the C ABI
is the same), so two builds that compute the same bits print the same text. No times. One line per
case, the digest over the bytes named:

  quads WxH guides           pos4, nrm4 and albedo4 of the two-quad scene of tests/test_denoise.py
  quads WxH FORMAT ...       the denoised frame's mapped bytes, row padding excluded: plain and
                             demodulated, 1, 3 and 5 iterations, filtered before the first map
                             (where it was rendered) and after a map (the upload path)
  cube W FORMAT N faces ...  yrtDenoiseCube over the Cornell box seen from inside
                             (tests/denoise_cube_ref.cube_args, 4 spp), 12 faces and the left eye's
                             6: no face mapped before the call, all of them, every second one
  loop W FORMAT ...          yrtDenoiseFrameBuffer face by face over the same 12 faces

at 40 x 24 and 38 x 24 (the RGB8 row padding) and at W = 48 and 38.

    YRT_LIB_DIR=... python tools/denoise_digest.py > digest.txt
"""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "yulio-raytracer_amd"), str(ROOT / "tests")]

POWER = 1 / 2.2
VARIANTS = (("plain", {}), ("demodulated", dict(demodulate=1, albedo_power=POWER)))
ITERATIONS = (1, 3, 5)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    import yrt
    from denoise_albedo_ref import mapped, pixels
    from test_denoise import FORMATS, Quads
    from test_denoise_cube import Cube

    d = yrt.Device(0)

    def frame(fb, fmt, w, h):
        return pixels(mapped(d, fb, fmt, w, h), fmt, w)

    q = Quads(d)
    cam, scene = q.ms.camera, q.ms.scene
    for w, h in ((40, 24), (38, 24)):
        print(f"quads {w}x{h} guides {sha(*d.render_guides(cam, scene, w, h), d.render_albedo(cam, scene, w, h))}",
              flush=True)
        for fmt in FORMATS:
            for name, kw in VARIANTS:
                for it in ITERATIONS:
                    for where in ("rendered", "mapped"):
                        fb = q.render(fmt, w, h)
                        if where == "mapped":
                            mapped(d, fb, fmt, w, h)
                        d.denoise(cam, scene, fb, iterations=it, **kw)
                        print(f"quads {w}x{h} {fmt:12s} {name:11s} x{it} {where:8s} {sha(frame(fb, fmt, w, h))}", flush=True)

    for w in (48, 38):
        c = Cube(d, w)
        for fmt in ("RGB8", "RGB_FLOAT32", "RGBA_FLOAT32"):
            for name, kw in VARIANTS:
                for it in ITERATIONS:
                    for faces in (range(12), range(6)):
                        for which, every in (("none", 0), ("all", 1), ("every 2nd", 2)):
                            fbs = c.job(fmt, faces)
                            for fb in fbs[every - 1::every] if every else ():
                                mapped(d, fb, fmt, w, w)
                            d.denoise_cube([c.cams[f] for f in faces], c.scene, fbs, iterations=it, **kw)
                            print(f"cube {w} {fmt:12s} {len(faces):2d} faces {name:11s} x{it} mapped {which:9s} "
                                  f"{sha(*(frame(fb, fmt, w, w) for fb in fbs))}", flush=True)
                    fbs = c.job(fmt)
                    for f, fb in enumerate(fbs):
                        d.denoise(c.cams[f], c.scene, fb, iterations=it, **kw)
                    print(f"loop {w} {fmt:12s} 12 faces {name:11s} x{it} {sha(*(frame(fb, fmt, w, w) for fb in fbs))}",
                          flush=True)
        c.s.close()
    d.close()


if __name__ == "__main__":
    main()
