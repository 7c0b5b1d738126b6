"""Scenes, rays and a brute-force reference for the ray-query kernel's edge tests
(tests/test_trace_edges.py; tests/test_trace_motion.py for moving geometry), and the scene, poses
and rays of the refit tests (tests/test_refit.py).

Everything is built through the device API (rtNewShape("trianglemesh"), positions, indices), so
the same builders serve the host-only device of the CPU tests and the MI355X.
"""
from __future__ import annotations

import numpy as np

F = np.float32
INF = np.float32(np.inf)


# ----------------------------------------------------------------------------- scene building
class MeshScene:
    """A committed scene of triangle meshes (one Matte material, optionally an ambient light) and a
    pinhole camera. meshes: [(positions (n, 3), indices (m, 3), cullBackFaces[, normals (n, 3)
    or None[, motions (n, 3) or None]])] in primitive-slot order; global triangle ids count through
    the meshes in that order. A mesh with motions (the "motions" float3 array: the vertex at ray
    time t is p + t * m) makes the scene a moving one; tri9 then holds the vertices at time 0 and
    mot9 their motions, zeros for the meshes without."""

    def __init__(self, dev, meshes, eye=(0, 0, -10), look=(0, 0, 0), up=(0, 1, 0), angle=60.0, light=None):
        from test_cpu_host import yrt_lookat
        d = self.dev = dev
        mat = self.mat = d.rtNewMaterial("Matte")
        d.rtSetFloat3(mat, "reflectance", 0.5, 0.5, 0.5)
        d.rtCommit(mat)
        self.scene = d.rtNewScene("default")
        self.meshes = []
        for slot, m in enumerate(meshes):
            pos, idx, cull = m[:3]
            mot = m[4] if len(m) > 4 else None
            self.meshes.append({"idx": np.ascontiguousarray(idx, np.int32), "cull": bool(cull),
                                "mot": None if mot is None else np.ascontiguousarray(mot, F)})
            self._set_mesh(slot, pos, m[3] if len(m) > 3 else None)
        self.has_motion = any(m["mot"] is not None for m in self.meshes)
        if light is not None:
            amb = d.rtNewLight("ambientlight")
            d.rtSetFloat3(amb, "L", light, light, light)
            d.rtCommit(amb)
            d.rtSetPrimitive(self.scene, len(meshes), d.rtNewLightPrimitive(amb))
        self.camera = d.rtNewCamera("pinhole")
        d.rtSetTransform(self.camera, "local2world", yrt_lookat(eye, look, up))
        d.rtSetFloat1(self.camera, "angle", angle)
        d.rtSetFloat1(self.camera, "aspectRatio", 1.0)
        d.rtCommit(self.camera)
        self.commit()

    def _set_mesh(self, slot, pos, nor, mat=None):
        """A new trianglemesh of the slot's indices and cull flag in the slot (not committed)."""
        d, m = self.dev, self.meshes[slot]
        m["pos"] = pos = np.ascontiguousarray(pos, F)
        m["nor"] = nor = None if nor is None else np.ascontiguousarray(nor, F)
        idx = m["idx"]
        mesh = d.rtNewShape("trianglemesh")
        d.rtSetArray(mesh, "positions", "float3", d.rtNewData("immutable", pos), len(pos), 12)
        if nor is not None:
            d.rtSetArray(mesh, "normals", "float3", d.rtNewData("immutable", nor), len(nor), 12)
        d.rtSetArray(mesh, "indices", "int3", d.rtNewData("immutable", idx), len(idx), 12)
        if m["mot"] is not None:
            assert m["mot"].shape == pos.shape
            d.rtSetArray(mesh, "motions", "float3", d.rtNewData("immutable", m["mot"]), len(pos), 12)
        if m["cull"]:
            d.rtSetBool1(mesh, "cullBackFaces", True)
        d.rtCommit(mesh)
        d.rtSetPrimitive(self.scene, slot, d.rtNewShapePrimitive(mesh, self.mat if mat is None else mat))

    def commit(self):
        """rtCommit of the scene; tri9, flags, info and blob follow the meshes as they are now."""
        self.dev.rtCommit(self.scene)
        self.tri9 = np.concatenate([m["pos"][m["idx"]].reshape(-1, 9) for m in self.meshes]).astype(F)  # v0 v1 v2 by id
        self.flags = np.concatenate([np.full(len(m["idx"]), 1 if m["cull"] else 0, np.uint32) for m in self.meshes])
        self.mot9 = np.concatenate([(np.zeros_like(m["pos"]) if m["mot"] is None else m["mot"])[m["idx"]].reshape(-1, 9)
                                    for m in self.meshes]).astype(F)
        if self.has_motion:
            # no -0.0 among the coordinates and motions: p + 0 * m is then p bit for bit
            for a in (self.tri9, self.mot9):
                assert not np.signbit(a[a == 0]).any()
        self.info = self.dev.scene_info(self.scene)
        self.blob = self.frame("debug")[1]

    def move(self, slot, positions, normals=None, commit=True):
        """The slot's mesh with new positions (and vertex normals; None keeps the mesh's own): a
        new trianglemesh with the same indices, material and cull flag, set into the slot, and the
        scene committed. commit=False leaves the commit to a later move or commit()."""
        self._set_mesh(slot, positions, self.meshes[slot]["nor"] if normals is None else normals)
        if commit:
            self.commit()

    def frame(self, renderer, spp=1, depth=2):
        """(renderer handle, frame blob) of a "debug" or "pathtracer" (maxDepth depth) renderer."""
        d = self.dev
        r = d.rtNewRenderer(renderer)
        if renderer == "pathtracer":
            d.rtSetInt1(r, "maxDepth", depth)
            d.rtSetFloat1(r, "tMaxShadowRay", 1e4)
        d.rtSetInt1(r, "sampler.spp", spp)
        d.rtCommit(r)
        return r, d.export_frame(r, self.camera, self.scene)

    def render(self, renderer, size):
        """The RGB_FLOAT32 frame of a renderer handle (default tone mapper, gamma 1)."""
        d = self.dev
        tm = d.rtNewToneMapper("default")
        d.rtCommit(tm)
        fb = d.rtNewFrameBuffer("RGB_FLOAT32", size, size)
        d.rtRenderFrame(renderer, self.camera, self.scene, tm, fb, 0)
        return d.framebuffer_array(fb, size, size, "RGB_FLOAT32")

    def bvh(self):
        """(quantized nodes, leaf records, bytes per leaf record) of the device's own tree."""
        _, tris = self.dev.export_bvh(self.scene)
        return self.dev.export_qbvh(self.scene), tris, self.info["triRecordBytes"]

    def leaf_records(self):
        """The device's leaf records by global triangle id: (v0, e1, e2 (T, 3), flags (T,))."""
        _, tris = self.dev.export_bvh(self.scene)
        rec = tris.reshape(-1, self.info["triRecordBytes"])[:, :48].copy().view(F).reshape(-1, 12)
        gid = rec[:, 3].copy().view(np.int32)
        first = np.unique(gid, return_index=True)[1]
        rec = rec[first]
        return rec[:, 0:3], rec[:, 4:7], rec[:, 8:11], rec[:, 7].copy().view(np.uint32)


# ----------------------------------------------------------------------------- brute force
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def brute_force(tri9, flags, org4, dir4, mot9=None, time=None, block=2048):
    """Every ray against every triangle, no BVH, float32 operation for operation as the kernel's
    tri_test_g and the oracle's tri_test state it (separate multiplies and adds, t = T / |den|,
    the cull flag). Returns (hit (n, 4) float32: t, u, v, id bits of the smallest (t, id) among
    the accepted triangles with tnear < t < tfar, or tfar, 0, 0, -1; occluded (n,) int32).
    time (n,), with mot9: every ray sees every triangle at its own time, the vertices p + time * m
    as a float32 product and then a float32 sum (two roundings, as tri_at and the oracle's trace
    state it), e1 = p0 - p1 and e2 = p2 - p0 from those. The block of rays then shrinks so that its
    (rays x triangles x 9) vertex array stays within 64 MB."""
    tri9 = np.ascontiguousarray(tri9, F)
    org4 = np.ascontiguousarray(org4, F)
    dir4 = np.ascontiguousarray(dir4, F)
    n, T = len(org4), len(tri9)
    if time is not None:
        time = np.ascontiguousarray(time, F)
        mot9 = np.ascontiguousarray(mot9, F)
        assert time.shape == (n,) and mot9.shape == tri9.shape
        block = max(1, min(block, (64 << 20) // (36 * max(T, 1))))
    cull = (np.asarray(flags)[None, :] & 1) != 0
    hit = np.zeros((n, 4), F)
    occ = np.zeros(n, np.int32)
    one = F(1.0)
    with np.errstate(all="ignore"):
        for b in range(0, n, block):
            if time is None:
                p = tri9[None, :, :]
            else:
                prod = time[b:b + block, None, None] * mot9[None, :, :]
                p = tri9[None, :, :] + prod
                assert prod.dtype == F and p.dtype == F
            v0 = [p[:, :, k] for k in range(3)]
            e1 = [p[:, :, k] - p[:, :, 3 + k] for k in range(3)]
            e2 = [p[:, :, 6 + k] - p[:, :, k] for k in range(3)]
            Ng = _cross(e1, e2)
            o = [org4[b:b + block, k, None] for k in range(3)]
            d = [dir4[b:b + block, k, None] for k in range(3)]
            tnear, tfar = org4[b:b + block, 3, None], dir4[b:b + block, 3, None]
            C = [v0[k] - o[k] for k in range(3)]
            R = _cross(d, C)
            den = _dot(Ng, d)
            absDen = np.abs(den)
            sgn = np.where(den < 0, -one, one).astype(F)
            U = _dot(R, e2) * sgn
            V = _dot(R, e1) * sgn
            ok = (den != 0) & (U >= 0) & (V >= 0) & (U + V <= absDen)
            ok &= ~(cull & ~(den > 0))
            t = (_dot(Ng, C) * sgn) / absDen
            ok &= (t > tnear) & (t < tfar)
            assert t.dtype == F and U.dtype == F
            tm = np.where(ok, t, INF)
            best = tm.min(axis=1, keepdims=True)
            win = np.argmax(ok & (tm == best), axis=1)       # the first = smallest id at the smallest t
            any_ = ok.any(axis=1)
            r = np.arange(len(win))
            h = hit[b:b + block]
            h[:, 0] = np.where(any_, t[r, win], tfar[:, 0])
            h[:, 1] = np.where(any_, (U / absDen)[r, win], 0)
            h[:, 2] = np.where(any_, (V / absDen)[r, win], 0)
            h[:, 3] = np.where(any_, win, -1).astype(np.int32).view(F)
            occ[b:b + block] = any_
    return hit, occ


# ----------------------------------------------------------------------------- deep-stack scene
CHAIN_N, CHAIN_R = 200, 0.93


def chain_mesh(n=CHAIN_N, r=CHAIN_R, seed=7):
    """A geometric chain along +x: triangle k has size s = r^k and lies around x = s; its box
    straddles the x axis in y and z by at least 0.2 s while the axis itself passes at least
    0.1 s beside it (rejection-sampled from a fixed seed). A ray along the axis enters every
    triangle's box and hits none, so from the fine end the nearest-first order stacks up the whole
    coarse rest of the chain."""
    rng = np.random.default_rng(seed)
    pos = []
    for k in range(n):
        s = r ** k
        while True:
            v = rng.uniform([0.75, -1.0, -1.0], [1.25, 1.0, 1.0], size=(3, 3))
            yz = v[:, 1:]
            if yz.min(0).max() > -0.2 or yz.max(0).min() < 0.2:
                continue
            # distance of the origin from the triangle projected along x
            dist = np.inf
            inside = True
            sign = 0.0
            for a in range(3):
                p, q = yz[a], yz[(a + 1) % 3]
                e = q - p
                c = e[0] * (-p[1]) - e[1] * (-p[0])
                if sign == 0.0:
                    sign = np.sign(c)
                elif np.sign(c) != sign:
                    inside = False
                tt = np.clip(np.dot(-p, e) / np.dot(e, e), 0.0, 1.0)
                dist = min(dist, float(np.linalg.norm(p + tt * e)))
            if inside or dist < 0.1:
                continue
            break
        pos.append(v * s)
    pos = np.concatenate(pos).astype(F)
    idx = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return pos, idx


CHAIN_WALL = 200  # global id of the backstop triangle


def chain_scene(dev, wall_motion=None):
    """The chain and, as a second mesh, a backstop triangle across the axis at x = 1.5 (beyond the
    coarse end): rays along the axis hit nothing but it. For +x rays from the fine end it is the
    farthest box, for -x any-hit rays from x = 2 the nearest, so either order pushes it first and
    pops it last: the hit is found only if the bottom of the stack survives the deep descent.
    The camera sits just before the fine end and looks along +x (24 degrees: the central rays run
    the whole chain, the outer ones hit its triangles).
    wall_motion: the backstop's three vertices get this motion (the chain itself stays unmoved),
    which makes the scene a moving one."""
    pos, idx = chain_mesh()
    w = 0.5
    wall = np.array([[1.5, -w, -w], [1.5, 2 * w, -w], [1.5, -w, 2 * w]], F)
    mot = None if wall_motion is None else np.tile(np.asarray(wall_motion, F), (3, 1))
    return MeshScene(dev, [(pos, idx, False), (wall, np.array([[0, 1, 2]], np.int32), False, None, mot)],
                     eye=(-1e-7, 0, 0), look=(1, 0, 0), up=(0, 1, 0), angle=24.0, light=2.0)


def chain_rays(tri9, n=4096, seed=11):
    """Rays for the chain, interleaved so that one wave holds every kind (kind = index % 4):
    0: from before the fine end along +x, 1: from x = 2 along -x, both within 1e-9 of the axis
    (far below the smallest triangle, 5e-7), a third of them tilted by up to 1e-10; a quarter of
    them with a range that ends before (kind 0: tfar 1.4) or starts behind (kind 1: tnear 0.6) the
    backstop; 2: incoherent rays from around the chain; 3: rays aimed at a triangle's centroid."""
    rng = np.random.default_rng(seed)
    org = np.zeros((n, 4), F)
    dr = np.zeros((n, 4), F)
    dr[:, 3] = INF
    i = np.arange(n)
    kind = i % 4
    jit = rng.uniform(-1e-9, 1e-9, size=(n, 3))
    a, b = kind == 0, kind == 1
    org[a, :3] = jit[a] * [0, 1, 1] + [-1e-7, 0, 0]
    dr[a, :3] = [1, 0, 0]
    org[b, :3] = jit[b] * [0, 1, 1] + [2.0, 0, 0]
    dr[b, :3] = [-1, 0, 0]
    tilt = (a | b) & (i % 3 == 0)
    dr[tilt, 1:3] = rng.uniform(-1e-10, 1e-10, size=(int(tilt.sum()), 2))
    short = (i // 4) % 4 == 3
    dr[a & short, 3] = 1.4
    org[b & short, 3] = 0.6
    c = kind == 2
    org[c, :3] = rng.uniform([-0.2, -1, -1], [1.5, 1, 1], size=(int(c.sum()), 3))
    v = rng.normal(size=(int(c.sum()), 3))
    dr[c, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    m = np.flatnonzero(kind == 3)
    cen = np.asarray(tri9, np.float64).reshape(-1, 3, 3).mean(1)
    o = rng.uniform([-0.2, -1, -1], [1.5, 1, 1], size=(len(m), 3))
    v = cen[rng.integers(0, len(cen), size=len(m))] - o
    org[m, :3] = o
    dr[m, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return org, dr, kind


CHAIN_WALL_MOTION = (0.0, 2.0, 0.0)  # the backstop's lower edge y = -0.5 + 2 * time reaches the axis at time 0.25


def moving_chain_scene(dev):
    """chain_scene with the backstop moving by CHAIN_WALL_MOTION: the axis passes through it only
    for time <= 0.25 (at exactly 0.25 its edge lies on the axis, and the rays' 1e-9 of jitter
    decides). Every query on this scene runs the moving-geometry kernels, while the chain, and with
    it the deep descent, is what it is in the static scene."""
    return chain_scene(dev, CHAIN_WALL_MOTION)


def chain_times(n=4096, seed=13):
    """A time per chain ray: half of them (drawn at random, so not in step with the rays' kinds)
    uniform in [0, 0.25), the rest uniform in (0.25, 1]; of every 16 the first is exactly 0, the
    second exactly 0.25 and the third exactly 1."""
    rng = np.random.default_rng(seed)
    low = rng.random(n) < 0.5
    t = np.where(low, rng.uniform(0.0, 0.25, n), 1.0 - rng.uniform(0.0, 0.75, n)).astype(F)
    i = np.arange(n)
    t[i % 16 == 0], t[i % 16 == 1], t[i % 16 == 2] = 0.0, 0.25, 1.0
    assert t.min() == 0 and t.max() == 1 and not np.signbit(t).any()
    return t


# ----------------------------------------------------------------------------- refill rays
def launch_chunk(n):
    """Rays per wave of a ray-query launch of n rays, from the launcher's constants: grid_for(n,
    YRT_TRACE_BLOCK, YRT_TRACE_GRID) blocks (kernels/pathtrace.hip) of YRT_TRACE_BLOCK / 64 waves,
    chunk = max(64, ceil(n / waves)) (kernels/k_trace.h). Returns (chunk, waves)."""
    import re
    from pathlib import Path
    k = Path(__file__).resolve().parent.parent / "yulio-raytracer_amd" / "csrc" / "kernels"
    grid = int(re.search(r"#define YRT_TRACE_GRID (\d+)", (k / "yrt_kernels.h").read_text()).group(1))
    block = int(re.search(r"#define YRT_TRACE_BLOCK (\d+)", (k / "yrt_traverse.h").read_text()).group(1))
    blocks = min(max((n + block - 1) // block, 1), grid)
    waves = blocks * (block // 64)
    return max(64, (n + waves - 1) // waves), waves


LONG_N = (1 << 20) + (1 << 19) + 37


def refill_base(org4, dir4, lo, hi):
    """A quarter of the rays (index % 4 == 1) made cheap or void, in turn: tfar < tnear, NaN tfar,
    an origin outside the scene box pointing away from it, tfar = 1e-3; an eighth (index % 8 == 0)
    gets the finite range 50. Ray costs inside one wave then differ by orders of magnitude."""
    org4, dir4 = org4.copy(), dir4.copy()
    i = np.arange(len(org4))
    dir4[i % 8 == 0, 3] = 50.0
    q, sub = i % 4 == 1, (i // 4) % 4
    m = q & (sub == 0)
    org4[m, 3], dir4[m, 3] = 1.0, 0.5
    dir4[q & (sub == 1), 3] = np.nan
    m = q & (sub == 2)
    ext = (np.asarray(hi) - np.asarray(lo)).astype(F)
    away = np.sign(dir4[m, :3])
    away[away == 0] = 1
    org4[m, :3] = np.where(away > 0, hi, lo).astype(F) + away.astype(F) * ext * F(0.25)
    dir4[q & (sub == 3), 3] = 1e-3
    return org4, dir4


# ----------------------------------------------------------------------------- exact-equality scene
EXACT_COPIES = 40
GRID = 6           # cells per side of the shuffled grid mesh
GRID_X = 32        # it spans [32, 38] x [0, 6] at z = 1
GRID_ID0 = 84      # its first global id


def grid_mesh():
    """A 6 x 6 grid of unit cells at z = 1, two triangles per cell, the triangles listed in a
    fixed shuffled order: up to six triangles with well separated centroids meet in a vertex, so
    the tree splits them spatially and its leaf order is not the id order."""
    n = GRID + 1
    pos = np.array([[GRID_X + i, j, 1] for j in range(n) for i in range(n)], F)
    tri = []
    for j in range(GRID):
        for i in range(GRID):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            tri += [[a, b, c], [a, c, d]]
    tri = np.array(tri, np.int32)
    return pos, tri[np.random.default_rng(5).permutation(len(tri))]


def exact_scene(dev):
    """Small integer coordinates: every product of the triangle test is exact.
    mesh 0 (ids 0..79): 40 coincident copies of the quad (0,0,1) (4,0,1) (4,4,1) (0,4,1), each as
      triangle A = (0,0) (4,0) (4,4) (even id, covers x >= y) and B = (0,0) (4,4) (0,4) (odd id,
      x <= y) sharing the diagonal. Ng = cross(e1, e2) = (0, 0, -16): den < 0 for rays going up.
    mesh 1 (ids 80, 81): the same quad at x + 8 with cullBackFaces: seen only by rays going down
      (den = dot(Ng, dir) > 0).
    mesh 2 (id 82: (6,0,0) (6,4,0) (6,0,4) in the plane x = 6; id 83: (0,6,0) (0,6,4) (4,6,0) in the
      plane y = 6): targets for rays along x and y.
    mesh 3 (ids 84..155): grid_mesh(). The builder keeps coincident triangles in id order, so among
      the copies of mesh 0 the first triangle accepted is also the winner; a ray through a grid
      vertex or edge ties up to six triangles at t = 1 that lie in different leaves in an order
      unrelated to their ids."""
    quad = np.array([[0, 0, 1], [4, 0, 1], [4, 4, 1], [0, 4, 1]], F)
    two = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    pos = np.tile(quad, (EXACT_COPIES, 1))
    idx = np.concatenate([two + 4 * k for k in range(EXACT_COPIES)])
    cq = quad + np.array([8, 0, 0], F)
    tp = np.array([[6, 0, 0], [6, 4, 0], [6, 0, 4], [0, 6, 0], [0, 6, 4], [4, 6, 0]], F)
    ti = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    gpos, gidx = grid_mesh()
    return MeshScene(dev, [(pos, idx, False), (cq, two, True), (tp, ti, False), (gpos, gidx, False)],
                     eye=(4, 2, -10), look=(4, 2, 1))


def _ray(o, d, tnear=0.0, tfar=np.inf):
    return [o[0], o[1], o[2], tnear, d[0], d[1], d[2], tfar]


def exact_rays():
    """(org4, dir4, expected id, expected t, name) of the hand-written cases. Expected id -1: no
    triangle accepted (not occluded); expected t is checked for hits."""
    up, dn = (0, 0, 1), (0, 0, -1)
    one_up, one_dn = np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0))
    rows = []

    def add(name, ray, tri, t=1.0):
        rows.append((name, ray, tri, t))

    # the shared diagonal (U = -0.0 for A, V + U = |den| for B), vertices, outer edges, interior
    for x in (1, 2, 3, 0.5):
        add(f"diagonal {x}", _ray((x, x, 0), up), 0)
    add("vertex 0,0", _ray((0, 0, 0), up), 0)
    add("vertex 4,4", _ray((4, 4, 0), up), 0)
    add("vertex 4,0", _ray((4, 0, 0), up), 0)
    add("vertex 0,4", _ray((0, 4, 0), up), 1)
    add("edge y=0", _ray((2, 0, 0), up), 0)
    add("edge x=4", _ray((4, 2, 0), up), 0)
    add("edge x=0", _ray((0, 2, 0), up), 1)
    add("edge y=4", _ray((2, 4, 0), up), 1)
    for x, y in ((-1, 1), (5, 2), (2, -0.5), (2, 4.5), (-0.25, -0.25)):
        add(f"outside {x},{y}", _ray((x, y, 0), up), -1)
    # through the coincident copies, from both sides: the smallest id of the 40 ties
    for k in range(7):
        for j in range(7):
            x, y = 0.5 * (k + 1), 0.5 * (j + 1)
            add(f"copies up {x},{y}", _ray((x, y, 0), up), 0 if x >= y else 1)
            add(f"copies down {x},{y}", _ray((x, y, 2), dn), 0 if x >= y else 1)
    # through the vertices and edge midpoints of the shuffled grid: the smallest id among the
    # triangles that hold the vertex (both ends of the edge), read off the index list
    gpos, gidx = grid_mesh()
    n = GRID + 1

    def holders(*verts):
        return GRID_ID0 + int(np.flatnonzero(np.all([(gidx == v).any(1) for v in verts], axis=0)).min())

    for j in range(n):
        for i in range(n):
            v = j * n + i
            add(f"grid vertex up {i},{j}", _ray((GRID_X + i, j, 0), up), holders(v))
            add(f"grid vertex down {i},{j}", _ray((GRID_X + i, j, 2), dn), holders(v))
            if i < GRID:
                add(f"grid edge x {i},{j}", _ray((GRID_X + i + 0.5, j, 0), up), holders(v, v + 1))
            if j < GRID:
                add(f"grid edge y {i},{j}", _ray((GRID_X + i, j + 0.5, 0), up), holders(v, v + n))
            if i < GRID and j < GRID:
                add(f"grid diagonal {i},{j}", _ray((GRID_X + i + 0.5, j + 0.5, 2), dn), holders(v, v + n + 1))
    # in the quad's plane (den == 0 for all 80 copies), on to the target behind it
    add("in plane +x", _ray((-1, 2, 1), (1, 0, 0)), 82, 7.0)
    add("in plane +y", _ray((3, 1, 1), (0, 1, 0)), 83, 5.0)
    add("in plane diagonal", _ray((-1, -1, 1), (1, 1, 0)), -1)
    # along each axis, +0 and -0 in the other components
    z = (0.0, -0.0)
    for a in z:
        for b in z:
            add(f"+z {a},{b}", _ray((3, 1, 0), (a, b, 1)), 0)
            add(f"-z {a},{b}", _ray((1, 3, 2), (a, b, -1)), 1)
            add(f"+x {a},{b}", _ray((5, 1, 0.5), (1, a, b)), 82)
            add(f"-x {a},{b}", _ray((7, 1, 0.5), (-1, a, b)), 82)
            add(f"+y {a},{b}", _ray((1, 5, 0.5), (a, 1, b)), 83)
            add(f"-y {a},{b}", _ray((1, 7, 0.5), (a, -1, b)), 83)
    # tiny direction components (safe_inv clamps them to +-1e-20) and a zero direction
    for a in (1e-30, -1e-30):
        for b in (1e-30, -1e-30):
            add(f"tiny {a},{b}", _ray((3, 1, 0), (a, b, 1)), 0)
    add("zero direction", _ray((3, 1, 0.5), (0, 0, 0)), -1)
    add("zero direction, on the quad", _ray((3, 1, 1), (0, 0, 0)), -1)
    # range edges around the hit at t = 1 (and t = 0.75, t = 0.5 with a direction of length 2)
    add("tfar == t", _ray((3, 1, 0), up, 0, 1.0), -1)
    add("tfar just above t", _ray((3, 1, 0), up, 0, one_up), 0)
    add("tfar just below t", _ray((3, 1, 0), up, 0, one_dn), -1)
    add("tnear == t", _ray((3, 1, 0), up, 1.0), -1)
    add("tnear just below t", _ray((3, 1, 0), up, one_dn), 0)
    add("tnear just above t", _ray((3, 1, 0), up, one_up), -1)
    add("tnear == tfar == t", _ray((3, 1, 0), up, 1.0, 1.0), -1)
    add("tfar inf", _ray((1, 3, 0), up, 0, np.inf), 1)
    add("tfar NaN", _ray((3, 1, 0), up, 0, np.nan), -1)
    add("tfar negative", _ray((3, 1, 0), up, 0, -1.0), -1)
    add("tfar < tnear around t", _ray((3, 1, 0), up, 1.5, 0.5), -1)
    add("t = 0.75", _ray((3, 1, 0.25), up), 0, 0.75)
    add("t = 0.75, tfar == t", _ray((3, 1, 0.25), up, 0, 0.75), -1)
    add("t = 0.5, |dir| = 2", _ray((3, 1, 0), (0, 0, 2)), 0, 0.5)
    add("t = 0.5, |dir| = 2, tnear == t", _ray((3, 1, 0), (0, 0, 2), 0.5), -1)
    # the culled quad: from the front (z > 1, looking down) and from behind
    add("culled front A", _ray((10, 1, 2), dn), 80)
    add("culled front B", _ray((9, 3, 2), dn), 81)
    add("culled front diagonal", _ray((10, 2, 2), dn), 80)
    add("culled back A", _ray((10, 1, 0), up), -1)
    add("culled back diagonal", _ray((10, 2, 0), up), -1)
    add("culled in plane", _ray((7.5, 1, 1), (1, 0, 0)), -1)
    r = np.array([x[1] for x in rows], F)
    return (np.ascontiguousarray(r[:, :4]), np.ascontiguousarray(r[:, 4:]), np.array([x[2] for x in rows], np.int32),
            np.array([x[3] for x in rows], F), [x[0] for x in rows])


def node_plane_rays(qnodes, lo, hi):
    """Rays up and down the z axis (the other direction components +0 and -0) from origins whose x
    (or y) lies exactly on an x (y) plane of the quantized nodes (origin + q * 2^e, common/
    yrt_qnode.h) inside the scene box [lo, hi]; the other coordinate steps through the box. The
    slab distance to that plane is then exactly 0 * 1e20."""
    rec = qnodes.reshape(-1, 64)
    origin = rec[:, 0:12].copy().view(F).astype(np.float64)
    exps = rec[:, 12:16].copy().view(np.uint32)[:, 0]
    child = rec[:, 16:32].copy().view(np.int32)
    words = rec[:, 32:48].copy().view(np.uint32)                             # lo x, hi x, lo y, hi y
    byte = (words[:, :, None] >> (8 * np.arange(4))[None, None, :]) & 0xFF
    org, dr = [], []
    for a in range(2):
        scale = 2.0 ** (((exps >> (8 * a)) & 0xFF).astype(np.int64) - 127)
        pl = origin[:, a, None, None] + byte[:, 2 * a:2 * a + 2, :] * scale[:, None, None]
        pl = np.unique(pl[np.broadcast_to((child != -1)[:, None, :], pl.shape)])
        pl = pl[(pl >= lo[a]) & (pl <= hi[a]) & (pl.astype(F).astype(np.float64) == pl)]
        other = np.arange(np.ceil(lo[1 - a]) + 0.25, hi[1 - a], 1.0)
        for p in pl:
            for o in other:
                xy = (p, o) if a == 0 else (o, p)
                for sx in (0.0, -0.0):
                    for sy in (0.0, -0.0):
                        org.append([xy[0], xy[1], 0.0, 0.0]); dr.append([sx, sy, 1.0, np.inf])
                        org.append([xy[0], xy[1], 2.0, 0.0]); dr.append([sx, sy, -1.0, np.inf])
    return np.array(org, F).reshape(-1, 4), np.array(dr, F).reshape(-1, 4)


# ----------------------------------------------------------------------------- moving geometry: exact sweeps
SWEEP_TIMES = (0.0, 0.25, 0.5, 0.75, 1.0)
SWEEP_COPIES = 40
(SW_QUAD_A, SW_QUAD_B, SW_ALONG, SW_COLLAPSE, SW_FLIP, SW_STATIC, SW_APPROACH, SW_APPROACH2, SW_STATIC2, SW_COVER_A,
 SW_COVER_B, SW_COPIES) = range(12)  # global triangle ids; the copies are SW_COPIES .. SW_COPIES + 79


def sweep_scene(dev):
    """Small integer coordinates, motions that are multiples of 4 and times in SWEEP_TIMES: every
    p + t * m and every product of the triangle test is exact. One case per band of y (10 apart),
    so no case's rays meet another's triangles. Ng = cross(e1, e2) with e1 = p0 - p1, e2 = p2 - p0.
    mesh 0 (ids 0, 1): exact_scene's quad (0,0,1) (4,0,1) (4,4,1) (0,4,1) as A (x >= y) and B,
      moving by (8, 0, 0): it spans x in [8 t, 8 t + 4].
    mesh 1 (id 2): (0,10,2) (4,10,2) (0,14,2) moving by (0, 0, 4), along the rays that go up: it
      lies at z = 2 + 4 t.
    mesh 2 (id 3): (0,20,1) (8,20,1) (0,28,1) whose third vertex moves by (0, -8, 0) onto the
      first: half the size at 0.5, collapsed (Ng = 0, den == 0) at exactly 1.
    mesh 3 (id 4), cullBackFaces: base (0,30,1) (8,30,1) moving by (0, 4, 0), apex (4,34,1) by
      (0, -4, 0): the apex crosses the base at exactly 0.5 (collinear, den == 0); before, Ng =
      (0, 0, -32 + 64 t) points down and the triangle is seen by rays going down, after, by rays
      going up. (4, 32) lies inside it at every time but 0.5.
    mesh 4 (id 5) static (0,40,1) (4,40,1) (0,44,1) and mesh 5 (id 6) the same at z = 3 moving by
      (0, 0, -4): coincident at exactly 0.5 (the tie goes to id 5), the moving one behind the
      static one before and in front of it after.
    mesh 6 (id 7) moving and mesh 7 (id 8) static: the same pair at y + 10 with the ids the other
      way round (the tie goes to the moving one).
    mesh 8 (ids 9, 10): the quad at y + 60, z = 1, moving by (8, 0, 0), under
    mesh 9 (ids 11 .. 90): 40 coincident static copies of the quad at y + 60, z = 2: the leaves of
      exact_scene's copies, walked by the moving-geometry kernels."""
    quad = np.array([[0, 0, 1], [4, 0, 1], [4, 4, 1], [0, 4, 1]], F)
    two = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    one = np.array([[0, 1, 2]], np.int32)

    def tri(y, z):
        return np.array([[0, y, z], [4, y, z], [0, y + 4, z]], F)

    def mot(*rows):
        return np.array(rows, F)

    cq = quad + F([0, 60, 0])
    copies = np.tile(quad + F([0, 60, 1]), (SWEEP_COPIES, 1))
    cidx = np.concatenate([two + 4 * k for k in range(SWEEP_COPIES)])
    meshes = [
        (quad, two, False, None, mot(*[(8, 0, 0)] * 4)),
        (tri(10, 2), one, False, None, mot(*[(0, 0, 4)] * 3)),
        (np.array([[0, 20, 1], [8, 20, 1], [0, 28, 1]], F), one, False, None, mot((0, 0, 0), (0, 0, 0), (0, -8, 0))),
        (np.array([[0, 30, 1], [8, 30, 1], [4, 34, 1]], F), one, True, None, mot((0, 4, 0), (0, 4, 0), (0, -4, 0))),
        (tri(40, 1), one, False),
        (tri(40, 3), one, False, None, mot(*[(0, 0, -4)] * 3)),
        (tri(50, 3), one, False, None, mot(*[(0, 0, -4)] * 3)),
        (tri(50, 1), one, False),
        (cq, two, False, None, mot(*[(8, 0, 0)] * 4)),
        (copies, cidx, False),
    ]
    return MeshScene(dev, meshes, eye=(4, 30, -40), look=(4, 30, 1))


def sweep_rays():
    """(org4, dir4, time, expected id, expected t, name) of the hand-written cases, each at the
    five SWEEP_TIMES in adjacent slots (so one wave holds the five times of a ray). Expected id -1:
    no triangle accepted; expected t is checked for hits."""
    up, dn = (0, 0, 1), (0, 0, -1)
    M = -1
    rows = []

    def add(name, ray, tris, ts=1.0):
        ts = [ts] * 5 if np.isscalar(ts) else ts
        assert len(tris) == 5 and len(ts) == 5
        for k, time in enumerate(SWEEP_TIMES):
            rows.append((f"{name} @ {time}", ray, time, tris[k], ts[k]))

    # the translated quad under (6, 1): not there yet, its edge x = 4 (A), A's interior, its edge
    # x = 0 (B), gone; under (6, 3) the interior is B's
    add("quad passes 6,1", _ray((6, 1, 0), up), [M, SW_QUAD_A, SW_QUAD_A, SW_QUAD_B, M])
    add("quad passes 6,3", _ray((6, 3, 0), up), [M, SW_QUAD_A, SW_QUAD_B, SW_QUAD_B, M])
    add("quad passes 6,1 from above", _ray((6, 1, 2), dn), [M, SW_QUAD_A, SW_QUAD_A, SW_QUAD_B, M])
    # its vertices (4, 0) and (0, 0) and the end of its diagonal pass (6, 0) and (6, 4)
    add("quad passes 6,0", _ray((6, 0, 0), up), [M, SW_QUAD_A, SW_QUAD_A, SW_QUAD_A, M])
    add("quad passes 6,4", _ray((6, 4, 0), up), [M, SW_QUAD_A, SW_QUAD_B, SW_QUAD_B, M])
    # the triangle moving along the ray: t = 2 + 4 time against tfar and tnear
    far = [2.0, 3.0, 4.0, 5.0, 6.0]
    add("along the ray", _ray((1, 11, 0), up), [SW_ALONG] * 5, far)
    add("along the ray, tfar 4", _ray((1, 11, 0), up, 0.0, 4.0), [SW_ALONG, SW_ALONG, M, M, M], far)
    add("along the ray, tnear 3", _ray((1, 11, 0), up, 3.0), [M, M, SW_ALONG, SW_ALONG, SW_ALONG], far)
    add("along the ray, tnear 2, tfar 6", _ray((1, 11, 0), up, 2.0, 6.0), [M, SW_ALONG, SW_ALONG, SW_ALONG, M], far)
    # against its motion, from above: t = 8 - (2 + 4 time)
    add("against the ray, tfar 4", _ray((1, 11, 8), dn, 0.0, 4.0), [M, M, M, SW_ALONG, SW_ALONG], [6.0, 5.0, 4.0, 3.0, 2.0])
    # the collapsing triangle: (1, 26) leaves it before 0.25, (1, 21) stays inside until it is
    # gone at 1; (0, 26) on the edge x = 0 that shrinks to y <= 26 at exactly 0.25
    add("collapse 1,26", _ray((1, 26, 0), up), [SW_COLLAPSE, M, M, M, M])
    add("collapse 1,21", _ray((1, 21, 0), up), [SW_COLLAPSE] * 4 + [M])
    add("collapse 0,26", _ray((0, 26, 0), up), [SW_COLLAPSE, SW_COLLAPSE, M, M, M])
    add("collapse 1,21 from above", _ray((1, 21, 2), dn), [SW_COLLAPSE] * 4 + [M])
    # the culled triangle that turns over, from below and from above
    add("flip from below", _ray((4, 32, 0), up), [M, M, M, SW_FLIP, SW_FLIP])
    add("flip from above", _ray((4, 32, 2), dn), [SW_FLIP, SW_FLIP, M, M, M])
    add("flip from below 3,32", _ray((3, 32, 0), up), [M, M, M, SW_FLIP, SW_FLIP])
    add("flip from above 5,32", _ray((5, 32, 2), dn), [SW_FLIP, SW_FLIP, M, M, M])
    # coincident at 0.5 only: from z = -2 the static one lies at 3, the moving one at 5 - 4 time
    meet_id = [SW_STATIC, SW_STATIC, SW_STATIC, SW_APPROACH, SW_APPROACH]
    meet_id2 = [SW_STATIC2, SW_STATIC2, SW_APPROACH2, SW_APPROACH2, SW_APPROACH2]
    meet_t = [3.0, 3.0, 3.0, 2.0, 1.0]
    add("meet, static id first", _ray((1, 41, -2), up), meet_id, meet_t)
    add("meet, moving id first", _ray((1, 51, -2), up), meet_id2, meet_t)
    # from above (z = 4): the static one at 3, the moving one at 1 + 4 time
    add("meet from above, static id first", _ray((1, 41, 4), dn), [SW_APPROACH, SW_APPROACH, SW_STATIC, SW_STATIC, SW_STATIC],
        [1.0, 2.0, 3.0, 3.0, 3.0])
    add("meet from above, moving id first", _ray((1, 51, 4), dn),
        [SW_APPROACH2, SW_APPROACH2, SW_APPROACH2, SW_STATIC2, SW_STATIC2], [1.0, 2.0, 3.0, 3.0, 3.0])
    # on the edge y = 40 and the vertex (0, 40) the two coincide in
    add("meet on an edge", _ray((2, 40, -2), up), meet_id, meet_t)
    add("meet on a vertex", _ray((0, 50, -2), up), meet_id2, meet_t)
    # under the copies: the moving quad covers (x, y) while x lies in [8 t, 8 t + 4]; then the ray
    # goes on into the 40 ties, of which the smallest id wins
    A, B = SW_COPIES, SW_COPIES + 1
    for x, y in ((3.5, 60.5), (0.5, 63.5), (3.5, 62.5), (1.5, 63.0), (2.0, 62.0), (3.0, 60.0), (0.5, 60.5)):
        a = x >= y - 60
        cover = [SW_COVER_A if (x - 8 * t) >= y - 60 else SW_COVER_B for t in SWEEP_TIMES]
        under = [8 * t <= x <= 8 * t + 4 for t in SWEEP_TIMES]
        assert any(under) and not all(under)
        add(f"copies {x},{y}", _ray((x, y, 0), up), [c if u else (A if a else B) for c, u in zip(cover, under)],
            [1.0 if u else 2.0 for u in under])
    r = np.array([x[1] for x in rows], F)
    return (np.ascontiguousarray(r[:, :4]), np.ascontiguousarray(r[:, 4:]), np.array([x[2] for x in rows], F),
            np.array([x[3] for x in rows], np.int32), np.array([x[4] for x in rows], F), [x[0] for x in rows])


# ----------------------------------------------------------------------------- moving geometry: a field
# The first field's per-vertex motions are uniform in [-FIELD_MOTION, FIELD_MOTION]^3. With 1 a stale time (the
# previous ray's) changes the occlusion flag of 1.6 % of the base rays only (the field stays one connected sheet: a
# ray aimed at it still meets a neighbour), with 4 of 3.8 %, with 8 of 5.3 %: the smallest of these that meets
# test_trace_motion's bar of 1/20. The closest hit changes for 34.5 %, 38.9 % and 43.3 %.
FIELD_MOTION = 8.0
FIELD_EYE, FIELD_LOOK = (12.0, 12.0, -6.0), (14.0, 0.0, 8.0)


def moving_field_scene(dev, light=2.0):
    """refit_meshes()' two height fields before REFIT_SCALE (the same seed and draws): the 23 x 17
    field (782 triangles, vertex normals) with per-vertex motions uniform in [-FIELD_MOTION,
    FIELD_MOTION]^3, the 9 x 31 field (558 triangles) static. Neighbouring vertices move apart and
    towards each other, so a triangle's shape, facing and box change over the frame, and the sheet
    folds over itself."""
    rng = np.random.default_rng(23)
    g0, i0, n0 = height_field(23, 17, (0, 0, 0), rng, normals=True)
    g1, i1, _ = height_field(9, 31, (30, 0, -6), rng)
    mot = np.random.default_rng(31).uniform(-FIELD_MOTION, FIELD_MOTION, g0.shape).astype(F) + F(0)
    return MeshScene(dev, [(g0, i0, False, n0, mot), (g1, i1, False)], eye=FIELD_EYE, look=FIELD_LOOK, light=light)


def moving_field_rays(S, n=1 << 16, seed=37):
    """(org4, dir4 with tfar inf, time, far) for moving_field_scene: times uniform in [0, 1], of
    every 16 the first exactly 0 and the second exactly 1; three quarters of the rays (index % 4
    != 3) aimed from 10 to 30 away at where a random triangle's centroid is at the ray's own
    time, jittered by 0.3, the rest from inside the scene's bounds in a random direction. far: 0.5
    to 1.5 times the distance to the aim (5 for the random rays), for cut-short variants."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    time = rng.uniform(0.0, 1.0, n).astype(F)
    time[i % 16 == 0], time[i % 16 == 1] = 0.0, 1.0
    org = np.zeros((n, 4), F)
    dr = np.zeros((n, 4), F)
    dr[:, 3] = INF
    far = np.full(n, 5.0)
    m = np.flatnonzero(i % 4 != 3)
    tri = rng.integers(0, len(S.tri9), len(m))
    p = S.tri9[tri].astype(np.float64) + time[m, None].astype(np.float64) * S.mot9[tri].astype(np.float64)
    aim = p.reshape(-1, 3, 3).mean(1) + rng.uniform(-0.3, 0.3, (len(m), 3))
    v = rng.normal(size=(len(m), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    dist = rng.uniform(10, 30, len(m))
    org[m, :3] = aim + v * dist[:, None]
    dr[m, :3] = -v
    far[m] = dist * rng.uniform(0.5, 1.5, len(m))
    m = np.flatnonzero(i % 4 == 3)
    org[m, :3] = rng.uniform(S.info["bboxLo"], S.info["bboxHi"], (len(m), 3))
    v = rng.normal(size=(len(m), 3))
    dr[m, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return org, dr, time, far.astype(F)


def moving_field_base(S):
    """The base set of the moving-field tests: moving_field_rays through refill_base (void and
    cheap rays mixed in). Returns (org4, dir4, time)."""
    org, dr, time, _ = moving_field_rays(S)
    org, dr = refill_base(org, dr, S.info["bboxLo"], S.info["bboxHi"])
    return org, dr, time


# ----------------------------------------------------------------------------- ray queries on the device
SENT_F = np.float32(-12345.0)
SENT_I = 0x5A5A5A5A


def ids(hit):
    return np.ascontiguousarray(hit[:, 3]).view(np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def query(dev, scene, org, dr, n=None, guard=64, time=None):
    """yrtIntersect and yrtOccluded on the first n rays into sentinel-filled outputs with `guard`
    spare elements: every slot < n written, the guard untouched. Returns (hit (n, 4), occ (n,)).
    time (one float per ray): the timed calls, yrtIntersectTimed and yrtOccludedTimed."""
    import torch
    n = len(org) if n is None else n
    o = torch.from_numpy(np.array(org[:max(n, 1)], np.float32)).cuda()
    d = torch.from_numpy(np.array(dr[:max(n, 1)], np.float32)).cuda()
    hit = torch.full((n + guard, 4), float(SENT_F), dtype=torch.float32, device="cuda")
    occ = torch.full((n + guard,), SENT_I, dtype=torch.int32, device="cuda")
    tp = None
    if time is not None:
        assert len(time) >= n
        t = torch.from_numpy(np.array(time[:max(n, 1)], np.float32)).cuda()
        tp = t.data_ptr()
    torch.cuda.synchronize()
    dev.intersect(scene, o.data_ptr(), d.data_ptr(), n, hit.data_ptr(), time_ptr=tp)
    dev.occluded(scene, o.data_ptr(), d.data_ptr(), n, occ.data_ptr(), time_ptr=tp)
    h, c = hit.cpu().numpy(), occ.cpu().numpy()
    assert (h[n:] == SENT_F).all() and (c[n:] == SENT_I).all(), "guard region written"
    assert (ids(h[:n]) != ids(np.full((1, 4), SENT_F))[0]).all() and (c[:n] != SENT_I).all(), "slot not written"
    return h[:n], c[:n]


def compare(h, c, ref_hit, ref_occ):
    """Triangle ids and occlusion flags bit-exact; t, u, v of hits bitwise equal (the same
    operations without contraction and a correctly rounded division)."""
    want = ids(ref_hit)
    bad = np.flatnonzero(ids(h) != want)
    assert len(bad) == 0, (len(bad), bad[:8], ids(h)[bad[:8]], want[bad[:8]])
    assert np.array_equal(c, ref_occ), np.flatnonzero(c != ref_occ)[:8]
    m = want >= 0
    for k, name in enumerate("tuv"):
        d = np.flatnonzero(bits(h[m, k]) != bits(ref_hit[m, k]))
        assert len(d) == 0, (name, len(d), h[m, k][d[:4]], ref_hit[m, k][d[:4]])


# ----------------------------------------------------------------------------- refit scene
# primitive slots of refit_meshes()
R_GRID, R_GRID2, R_QUAD, R_SLIVERS, R_ZERO, R_FAR, R_TINY, R_POINT = range(8)
REFIT_SCALE = 16.0  # of the grids, the quad and the slivers: child boxes overlap by more than the spatial
#                     splits' threshold, 1e-5 of the root box's area, which R_FAR makes large
REFIT_EYE, REFIT_LOOK = (264.0, 1312.0, -964.0), (264.0, 912.0, -564.0)  # on the first grid under refit_pose_a


def height_field(nx, nz, at, rng, normals=False):
    """nx x nz quads (two triangles each) over a jittered unit grid in x and z from `at`, with
    random heights in [0, 1.5]; normals: unit vertex normals tilted at random off +y."""
    x, z = np.meshgrid(np.arange(nx + 1.0), np.arange(nz + 1.0))
    n = x.size
    pos = np.stack([x.ravel() + rng.uniform(-0.3, 0.3, n), rng.uniform(0.0, 1.5, n),
                    z.ravel() + rng.uniform(-0.3, 0.3, n)], 1) + np.asarray(at, np.float64)
    tri = []
    for j in range(nz):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            tri += [[a, b, c], [a, c, d]]
    nor = None
    if normals:
        nor = np.stack([rng.uniform(-0.4, 0.4, n), np.ones(n), rng.uniform(-0.4, 0.4, n)], 1)
        nor = (nor / np.linalg.norm(nor, axis=1, keepdims=True)).astype(F)
    return pos.astype(F) + F(0), np.array(tri, np.int32), nor


def refit_meshes(seed=23):
    """The refit tests' scene, in slot order (fixed seed; no coordinate is -0.0, so a minimum is
    the same bits in whatever order it is taken; sizes before REFIT_SCALE, which applies to the
    first four):
      R_GRID: a 23 x 17 height field (782 triangles, not a multiple of 64) with vertex normals;
      R_GRID2: a 9 x 31 height field (558 triangles); R_QUAD: one quad;
      R_SLIVERS: 40 triangles 25 long and 0.02 wide across both grids, cullBackFaces;
      R_ZERO: 5 triangles of all-zero vertices; R_FAR: a 2 x 2 field at x = 1e6;
      R_TINY: a 2 x 2 field scaled by 1e-30; R_POINT: a triangle collapsed to a point beside one
      of negative coordinates."""
    rng = np.random.default_rng(seed)
    g0, i0, n0 = height_field(23, 17, (0, 0, 0), rng, normals=True)
    g1, i1, _ = height_field(9, 31, (30, 0, -6), rng)
    q, iq, _ = height_field(1, 1, (-5, 1, 2), rng)
    a = rng.uniform([0, 0, 0], [40, 2, 18], size=(40, 3))
    u = rng.normal(size=(40, 3)) * [1, 0.1, 1]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, [0, 1, 0])
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    sl = np.stack([a, a + 25.0 * u, a + 0.02 * w], 1).reshape(-1, 3).astype(F) + F(0)
    isl = np.arange(120, dtype=np.int32).reshape(40, 3)
    g0, g1, q, sl = (p * F(REFIT_SCALE) for p in (g0, g1, q, sl))
    far, ifar, _ = height_field(2, 2, (1e6, 0, 0), rng)
    tiny, itiny, _ = height_field(2, 2, (1, 1, 1), rng)
    tiny = tiny * F(1e-30)
    pt = np.array([[3, -2, 4]] * 3 + [[-7, -3, -2], [-6, -3, -2], [-7, -2, -3]], F)
    ipt = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    meshes = [(g0, i0, False, n0), (g1, i1, False), (q, iq, False), (sl, isl, True),
              (np.zeros((15, 3), F), np.arange(15, dtype=np.int32).reshape(5, 3), False),
              (far, ifar, False), (tiny, itiny, False), (pt, ipt, False)]
    for m in meshes:
        assert not np.signbit(m[0][m[0] == 0]).any()
    return meshes


def refit_scene(dev):
    """refit_meshes() under an ambient light; the camera looks at where refit_pose_a puts R_GRID."""
    return MeshScene(dev, refit_meshes(), eye=REFIT_EYE, look=REFIT_LOOK, light=2.0)


def _turn(pos, nor, axis, angle, shift):
    """pos turned about its centroid (Rodrigues' formula) and shifted, nor turned with it."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    p = np.asarray(pos, np.float64)
    c = p.mean(0)
    out = ((p - c) @ R.T + c + np.asarray(shift, np.float64)).astype(F) + F(0)
    return out, None if nor is None else (np.asarray(nor, np.float64) @ R.T).astype(F) + F(0)


def refit_pose_a(S):
    """(a): R_GRID turned by 0.7 rad about (1, 2, 3) and shifted by 900 in y and -700 in z, out of
    the built scene's bounds."""
    m = S.meshes[R_GRID]
    S.move(R_GRID, *_turn(m["pos"], m["nor"], (1, 2, 3), 0.7, (80, 900, -700)))


def refit_pose_b(S):
    """(b): the quad, the slivers and the second grid moved in one commit."""
    S.move(R_QUAD, _turn(S.meshes[R_QUAD]["pos"], None, (0, 0, 1), 2.0, (140, -25, 50))[0], commit=False)
    S.move(R_SLIVERS, _turn(S.meshes[R_SLIVERS]["pos"], None, (0, 1, 0), 0.5, (0, 60, 0))[0], commit=False)
    S.move(R_GRID2, S.meshes[R_GRID2]["pos"] + F([8.5, -50, 4.25]))


def refit_pose_c(S):
    """(c): the second grid collapsed to one point."""
    S.move(R_GRID2, np.tile(F([504.5, 36.25, 114.125]), (len(S.meshes[R_GRID2]["pos"]), 1)))


def refit_pose_d(S):
    """(d): R_GRID carried to coordinates near -3e5 (float spacing there: 1/32)."""
    S.move(R_GRID, S.meshes[R_GRID]["pos"] + F([-3e5, -3e5, -3e5]))


REFIT_POSES = (refit_pose_a, refit_pose_b, refit_pose_c, refit_pose_d)


def refit_rays(S, old9, new9, n, seed=17):
    """Rays for a scene S in which one mesh moved (old9 -> new9, its triangles before and after),
    interleaved by index % 3: 0: aimed at a triangle of new9, 1: at one of old9 (from 160 to 480
    away, the aim jittered by 3), 2: from a point inside the scene's bounds as they are now, short
    of R_FAR (whose 1e6 would leave the rest a speck in the box), in a random direction or, every
    second one, towards a vertex of the scene. Returns (org4, dir4 with tfar inf, dir4 with half of the rays
    cut at a finite tfar: 0.5 to 1.5 times the distance to the aim, 300 for kind 2)."""
    rng = np.random.default_rng(seed)
    org = np.zeros((n, 4), F)
    dr = np.zeros((n, 4), F)
    dr[:, 3] = INF
    far = np.full(n, 300.0)
    kind = np.arange(n) % 3
    for k, t9 in ((0, new9), (1, old9)):
        m = np.flatnonzero(kind == k)
        cen = np.asarray(t9, np.float64).reshape(-1, 3, 3).mean(1)
        aim = cen[rng.integers(0, len(cen), len(m))] + rng.uniform(-3, 3, (len(m), 3))
        v = rng.normal(size=(len(m), 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        dist = rng.uniform(160, 480, len(m))
        org[m, :3] = aim + v * dist[:, None]
        dr[m, :3] = -v
        far[m] = dist * rng.uniform(0.5, 1.5, len(m))
    m = np.flatnonzero(kind == 2)
    v9 = np.concatenate([m["pos"] for k, m in enumerate(S.meshes) if k != R_FAR]).astype(np.float64)
    org[m, :3] = rng.uniform(v9.min(0), v9.max(0), (len(m), 3))
    v = rng.normal(size=(len(m), 3))
    aimed = np.arange(len(m)) % 2 == 1                   # every second one towards some vertex, not quite at it
    v[aimed] = v9[rng.integers(0, len(v9), int(aimed.sum()))] + rng.uniform(-3, 3, (int(aimed.sum()), 3)) - org[m[aimed], :3]
    dr[m, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    cut = dr.copy()
    half = (np.arange(n) // 3) % 2 == 0
    cut[half, 3] = far[half]
    return org, dr, cut
