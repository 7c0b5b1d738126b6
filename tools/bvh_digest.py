#!/usr/bin/env python3
"""sha256 of what a scene commit gives on the host, to compare two builds of the library byte for
byte.

On the host-only device every scene below is committed with "default" (YRT_SBVH unset), "default"
with YRT_SBVH=1 and "morton" (the host loop); the first digest is over the float nodes, the leaf
records and the quantized nodes (tests/test_refit._exports). One line per scene and setting:

    name  builder  YRT_SBVH  sha256  numNodes  numTriRefs  bvhDepth  (builder, fallback)
    pools sha256  frame sha256  info sha256

pools: the four yrtDebugTexturePool tables (images, textures, texels, quads); frame: the
yrtExportFrame blob of a session's scene ("-" for a bare mesh); info: yrtGetSceneInfo without
buildSeconds. The sessions are C2 to C5 and sphere_motion, so 8-bit textures, a float HDRI image,
light-bearing primitives and moving geometry are in the set.

No times, no GPU: two builds that commit the same scenes print the same text.

    python tools/bvh_digest.py [--tree CHECKOUT] > digest.txt

--tree: the built checkout whose library, package and test scenes are used (default: this one).
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

SETTINGS = (("default", None), ("default", "1"), ("morton", None))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
    root = Path(ap.parse_args().tree).resolve()
    for p in (root, root / "yulio-raytracer_amd", root / "tests"):
        sys.path.insert(0, str(p))
    import test_morton_build as tm
    import trace_scenes as ts
    import yrt
    from test_refit import _exports
    from yrt import frederick, standin

    def mesh(pos, idx):
        return lambda dev: ts.MeshScene(dev, [(pos, idx, False)])

    one = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    pos, idx, _ = ts.height_field(257, 256, (0, 0, 0), np.random.default_rng(41))
    scenes = dict(tm.SCENES)
    scenes["staircase"] = tm.staircase_scene
    scenes["one_triangle"] = mesh(one, np.arange(3, dtype=np.int32).reshape(1, 3))
    scenes["field_2^17"] = mesh(pos, np.ascontiguousarray(idx[:1 << 17]))
    small = ["-size", "32", "32", "-spp", "1"]
    sessions = {"sphere_motion": ["-c", str(root / "scenes" / "samples" / "sphere_motion.ecs")] + small,
                "C2": ["-c", str(root / "scenes" / "cornell_box_spheres.ecs")] + small,
                "C3": ["-i", str(standin.write_xml())] + standin.C3_ARGS + small,
                "C4": ["-i", str(root / "scenes" / "test_stereo.xml"), "-c", str(root / "scenes" / "test_stereo_view.ecs"),
                       "-stereo"] + small,
                "C5": ["-fprCollada", "-i", str(frederick.write_dae()), "-stereo"] + small}

    dev = yrt.Device(host=True)

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    def line(name, builder, sbvh, scene, exports, frame=None):
        info, bi = dev.scene_info(scene), dev.scene_build_info(scene)
        pools = dev.debug_texture_pools(scene)
        rest = sorted((k, v) for k, v in info.items() if k != "buildSeconds")
        print(f"{name:14s} {builder:8s} YRT_SBVH={sbvh or '-'} {sha(*exports)} nodes {info['numNodes']} "
              f"refs {info['numTriRefs']} bvhDepth {info['bvhDepth']} builder {bi['builder']} "
              f"fallback {bi['fallback']} pools {sha(*(pools[k] for k in ('images', 'textures', 'texels', 'quads')))} "
              f"frame {sha(frame) if frame is not None else '-'} info {sha(repr(rest).encode())}", flush=True)

    for builder, sbvh in SETTINGS:
        os.environ.pop("YRT_SBVH", None)
        if sbvh:
            os.environ["YRT_SBVH"] = sbvh
        for name, make in scenes.items():
            S = tm.morton(make(dev), builder)
            line(name, builder, sbvh, S.scene, _exports(S))
        for name, args in sessions.items():
            s = yrt.Session(args + ["-builder", builder], device=dev)
            scene = s.info()["scene"]
            line(name, builder, sbvh, scene, (*dev.export_bvh(scene), dev.export_qbvh(scene)), s.export_frame())
            s.close()
    dev.close()


if __name__ == "__main__":
    main()
