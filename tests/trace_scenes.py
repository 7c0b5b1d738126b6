"""Scenes, rays and a brute-force reference for the ray-query kernel's edge tests
(tests/test_trace_edges.py).

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
    pinhole camera. meshes: [(positions (n, 3), indices (m, 3), cullBackFaces)] in primitive-slot
    order; global triangle ids count through the meshes in that order."""

    def __init__(self, dev, meshes, eye=(0, 0, -10), look=(0, 0, 0), up=(0, 1, 0), angle=60.0, light=None):
        from test_cpu_host import yrt_lookat
        d = self.dev = dev
        mat = d.rtNewMaterial("Matte")
        d.rtSetFloat3(mat, "reflectance", 0.5, 0.5, 0.5)
        d.rtCommit(mat)
        self.scene = d.rtNewScene("default")
        tri9, flags = [], []
        for slot, (pos, idx, cull) in enumerate(meshes):
            pos = np.ascontiguousarray(pos, F)
            idx = np.ascontiguousarray(idx, np.int32)
            mesh = d.rtNewShape("trianglemesh")
            dp, di = d.rtNewData("immutable", pos), d.rtNewData("immutable", idx)
            d.rtSetArray(mesh, "positions", "float3", dp, len(pos), 12)
            d.rtSetArray(mesh, "indices", "int3", di, len(idx), 12)
            if cull:
                d.rtSetBool1(mesh, "cullBackFaces", True)
            d.rtCommit(mesh)
            d.rtSetPrimitive(self.scene, slot, d.rtNewShapePrimitive(mesh, mat))
            tri9.append(pos[idx].reshape(-1, 9))
            flags.append(np.full(len(idx), 1 if cull else 0, np.uint32))
        if light is not None:
            amb = d.rtNewLight("ambientlight")
            d.rtSetFloat3(amb, "L", light, light, light)
            d.rtCommit(amb)
            d.rtSetPrimitive(self.scene, len(meshes), d.rtNewLightPrimitive(amb))
        d.rtCommit(self.scene)
        self.tri9 = np.concatenate(tri9).astype(F)       # (T, 9): v0 v1 v2 by global id
        self.flags = np.concatenate(flags)                # (T,): bit 0 = cullBackFaces
        self.camera = d.rtNewCamera("pinhole")
        d.rtSetTransform(self.camera, "local2world", yrt_lookat(eye, look, up))
        d.rtSetFloat1(self.camera, "angle", angle)
        d.rtSetFloat1(self.camera, "aspectRatio", 1.0)
        d.rtCommit(self.camera)
        self.info = d.scene_info(self.scene)
        self.blob = self.frame("debug")[1]

    def frame(self, renderer, spp=1):
        """(renderer handle, frame blob) of a "debug" or "pathtracer" (depth 2) renderer."""
        d = self.dev
        r = d.rtNewRenderer(renderer)
        if renderer == "pathtracer":
            d.rtSetInt1(r, "maxDepth", 2)
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


def brute_force(tri9, flags, org4, dir4, block=2048):
    """Every ray against every triangle, no BVH, float32 operation for operation as the kernel's
    tri_test_g and the oracle's tri_test state it (separate multiplies and adds, t = T / |den|,
    the cull flag). Returns (hit (n, 4) float32: t, u, v, id bits of the smallest (t, id) among
    the accepted triangles with tnear < t < tfar, or tfar, 0, 0, -1; occluded (n,) int32)."""
    tri9 = np.ascontiguousarray(tri9, F)
    org4 = np.ascontiguousarray(org4, F)
    dir4 = np.ascontiguousarray(dir4, F)
    n, T = len(org4), len(tri9)
    v0 = [tri9[None, :, k] for k in range(3)]
    e1 = [tri9[None, :, k] - tri9[None, :, 3 + k] for k in range(3)]
    e2 = [tri9[None, :, 6 + k] - tri9[None, :, k] for k in range(3)]
    Ng = _cross(e1, e2)
    cull = (np.asarray(flags)[None, :] & 1) != 0
    hit = np.zeros((n, 4), F)
    occ = np.zeros(n, np.int32)
    one = F(1.0)
    with np.errstate(all="ignore"):
        for b in range(0, n, block):
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


def chain_scene(dev):
    """The chain and, as a second mesh, a backstop triangle across the axis at x = 1.5 (beyond the
    coarse end): rays along the axis hit nothing but it. For +x rays from the fine end it is the
    farthest box, for -x any-hit rays from x = 2 the nearest, so either order pushes it first and
    pops it last: the hit is found only if the bottom of the stack survives the deep descent.
    The camera sits just before the fine end and looks along +x (24 degrees: the central rays run
    the whole chain, the outer ones hit its triangles)."""
    pos, idx = chain_mesh()
    w = 0.5
    wall = np.array([[1.5, -w, -w], [1.5, 2 * w, -w], [1.5, -w, 2 * w]], F)
    return MeshScene(dev, [(pos, idx, False), (wall, np.array([[0, 1, 2]], np.int32), False)],
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
