"""The scene builder "morton" (rtSetString(scene, "builder", "morton"): an LBVH over 63-bit Morton
keys collapsed to the 4-wide nodes; common/yrt_lbvh.h, yrt_bvh4.h, kernels/k_bvh_build.h, the host
loop in device/bvh_build.cpp) against what the triangles and the topology determine
(tests/refit_ref.py, test_refit._check_state) and against brute force. Hits do not depend on the
tree, so nothing here has a tolerance: exports are compared byte for byte, hits bit for bit.

The CPU tests run the builder's host loop (builder 2) on the host device; the GPU tests require the
kernels (builder 1) to give the host loop's bytes, on every run.

Measured on the CPU (host loop against the host SAH builder; node visits of 4096 rays through the
quantized nodes, oracle.count_visits):
  refit_scene (1405 triangles, refit_rays): 125 nodes against 326, bvhDepth 23 against 22, sahCost
    0.0374 against 0.0098 (ratio 3.809; R_FAR at x = 1e6 makes the root box huge and the absolute
    figures small), 24.60 node visits per ray against 17.38 (ratio 1.416)
  C3 stand-in (67 472 triangles, incoherent rays from inside the bounds): 5 629 nodes against
    16 725, bvhDepth 28 against 31, sahCost 48.47 against 27.95 (ratio 1.734), 11.23 node visits per
    ray against 11.17 (ratio 1.005; triangle visits 9.88 against 2.50: the leaves are fuller)
  staircase: the morton tree's stack bound is 87 (> 63; computed by the host loop with the limit
    lifted), so the commit falls back (fallback 3) to the SAH builder, whose bound is 39.
Measured on the MI355X: every export of the kernels' trees equalled the host loop's on the first
run, two builds in a row were byte-identical, frames were bit-identical between the builders; the
2^17 + 37-triangle build took 0.82 ms of kernel time (DESIGN.md §10 has the build and frame times).
"""
import numpy as np
import pytest

import oracle
import refit_ref as rr
import trace_scenes as ts
from test_refit import _check_state, _exports, _refit_all_poses

F = np.float32


# ----------------------------------------------------------------------------- scenes
def morton(S, builder="morton"):
    """The scene re-committed with another builder (a commit that changes the builder rebuilds)."""
    S.dev.rtSetString(S.scene, "builder", builder)
    S.commit()
    return S


def soup(n, seed=3):
    """n small triangles scattered in [0, 10]^3 (fixed seed)."""
    rng = np.random.default_rng(seed + n)
    p = rng.uniform(0, 10, (n, 1, 3)) + rng.uniform(-0.4, 0.4, (n, 3, 3))
    return p.reshape(-1, 3).astype(F) + F(0), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def soup_scene(dev, n):
    pos, idx = soup(n)
    return ts.MeshScene(dev, [(pos, idx, False)], eye=(5, 5, -20), look=(5, 5, 5))


def line_scene(dev, n=37):
    """n triangles whose box centres lie on one line along x: the keys use one axis only."""
    x = np.arange(n, dtype=np.float64)[:, None, None] * 1.5
    tri = np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, -0.5], [-0.5, 0.5, 0.5]])[None] + x * np.array([1.0, 0, 0])
    return ts.MeshScene(dev, [(tri.reshape(-1, 3).astype(F), np.arange(3 * n, dtype=np.int32).reshape(n, 3), False)],
                        eye=(20, 0, -40), look=(20, 0, 0))


STAIR_E = 2.0 ** 21


def _small_tri(p):
    """A triangle whose box is p -+ 0.25 on every axis: its box centre is p exactly."""
    p = np.asarray(p, np.float64)
    q = 0.25
    return np.stack([p - q, p + q, p + [q, -q, -q]])


def staircase_scene(dev):
    """Keys that are the single bits 2^0 .. 2^62 (triangle j: the coordinate 2^(j // 3) of 2^21 on
    axis 2 - j % 3, the others 0), one triangle at the far corner (2^21 on every axis: it fixes the
    centroid bounds, so a coordinate is its own 21-bit number) and 4096 identical triangles at the
    origin. The radix tree is a caterpillar: every level splits one key off, every 4-wide node
    keeps three leaves and one inner child, and the stack bound grows by 3 per 4-wide level."""
    tris = []
    for j in range(63):
        p = np.zeros(3)
        p[2 - j % 3] = 2.0 ** (j // 3)
        tris.append(_small_tri(p))
    tris.append(_small_tri([STAIR_E] * 3))
    tris += [_small_tri([0, 0, 0])] * 4096
    pos = np.concatenate(tris).astype(F) + F(0)
    return ts.MeshScene(dev, [(pos, np.arange(len(pos), dtype=np.int32).reshape(-1, 3), False)],
                        eye=(0, 0, -100), look=(0, 0, 0))


def nan_scene(dev):
    pos, idx = soup(20)
    pos[31, 1] = np.nan
    return ts.MeshScene(dev, [(pos, idx, False)], eye=(5, 5, -20), look=(5, 5, 5))


def big_field():
    """A height field of 2^17 + 37 triangles (beyond what one block of a sort or scan holds)."""
    n = (1 << 17) + 37
    pos, idx, _ = ts.height_field(257, 256, (0, 0, 0), np.random.default_rng(41))
    return pos, np.ascontiguousarray(idx[:n])


SMALL = (2, 3, 5, 9, 63, 64, 65, 257)
SCENES = {"refit": ts.refit_scene, "exact": ts.exact_scene, "chain": ts.chain_scene, "line": line_scene}
SCENES.update({f"soup{n}": (lambda dev, n=n: soup_scene(dev, n)) for n in SMALL})


# ----------------------------------------------------------------------------- restatements
def np_keys(tri9):
    """The 63-bit key of every triangle from its nine floats, in float32 as the builder states it:
    c = 0.5 (lo + hi), q = min(2^21 - 1, (int)((c - lo_c) * (2^21 / (hi_c - lo_c)))), 0 on an axis
    without extent; x, y, z interleaved from bit 62 down."""
    v = np.ascontiguousarray(tri9, F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        c = F(0.5) * (v.min(1) + v.max(1))
        assert c.dtype == F
        key = np.zeros(len(c), np.uint64)
        for a in range(3):
            lo, hi = c[:, a].min(), c[:, a].max()
            q = np.zeros(len(c), np.uint64)
            if hi > lo:
                f = (c[:, a] - lo) * (F(2097152.0) / (hi - lo))
                assert f.dtype == F
                q = np.where(f > 0, np.minimum(f, F(2097151.0)), F(0)).astype(np.int64).astype(np.uint64)
            for b in range(21):
                key |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return key


def stack_bound(children):
    """The worst-case traversal stack: the largest sum of (children - 1) along a root path."""
    above = np.zeros(len(children), np.int64)
    worst = 0
    for ni in range(len(children)):                    # a child's index is above its parent's
        c = children[ni][children[ni] != -1]
        here = above[ni] + len(c) - 1
        worst = max(worst, int(here))
        inner = c[(c & 31) == 0] >> 5
        assert (inner > ni).all()
        above[inner] = here
    return worst


def check_structure(S):
    """Leaves of 1..8 triangles, the stack bound the builder reports, keys ordered along the
    leaves with ids ascending inside equal keys."""
    nodes, tris, _ = _exports(S)
    _, children, _ = rr.split_nodes(nodes)
    valid = children != -1
    assert valid[0].sum() >= 2, "the root is an inner node"
    cnt = children[valid] & 31
    assert cnt.max() <= 8 and (cnt[cnt > 0] >= 1).all()
    leaves = children[valid & ((children & 31) > 0)]
    assert (leaves & 31).sum() == len(S.tri9), "every leaf slot in one leaf"
    assert stack_bound(children) == S.info["bvhDepth"] <= 63
    gid = rr.split_tris(tris, S.info["triRecordBytes"])[3][:, 0]
    k = np_keys(S.tri9)[gid]
    assert (k[1:] >= k[:-1]).all(), "keys not ordered along the leaves"
    same = k[1:] == k[:-1]
    assert (gid[1:][same] > gid[:-1][same]).all(), "equal keys not in id order"
    return k


def visits(S, org, dr):
    """(mean node visits, hit) of the kernel-order traversal of the scene's quantized nodes."""
    nodes, tris, q = _exports(S)
    nv, _, hit = oracle.count_visits(nodes, tris, org, dr, tri_bytes=S.info["triRecordBytes"], qnodes=q)
    return nv / len(org), hit


# ============================================================================= CPU
@pytest.mark.parametrize("name", list(SCENES))
def test_host_loop_tree(host_device, name):
    """The host loop's tree of every scene: each triangle in exactly one leaf, records, boxes and
    quantized bytes exact, containment (_check_state); the structure; builder 2 without fallback;
    another tree than the default builder's."""
    S = SCENES[name](host_device)
    default = _exports(S)
    assert host_device.scene_build_info(S.scene)["builder"] == 0
    morton(S)
    bi = host_device.scene_build_info(S.scene)
    assert (bi["builder"], bi["fallback"]) == (2, 0), bi
    assert bi["msBuild"] > 0 and bi["msKernels"] == 0 and bi["sahCost"] >= 0
    assert _check_state(S) == 0
    k = check_structure(S)
    if name == "exact":
        assert (np.bincount(np.unique(k, return_inverse=True)[1]) >= 40).any(), "no run of equal keys"
    if name == "line":
        assert (k & np.uint64(0x36DB6DB6DB6DB6DB)).max() == 0 and len(np.unique(k)) == len(k), "y or z bits set"
    if len(S.tri9) > 8:
        mine = _exports(S)
        assert len(mine[0]) != len(default[0]) or not np.array_equal(mine[0], default[0]), "the default builder's tree"
    # the same input gives the same bytes again
    again = _exports(morton(S))
    for a, b in zip(_exports(S), again):
        assert np.array_equal(a, b)


def test_default_is_untouched(host_device, monkeypatch):
    """"default", another string and an unset property are the host SAH builder; switching back
    from "morton" gives the default tree again; YRT_BUILDER=morton makes "default" mean morton."""
    S = ts.refit_scene(host_device)
    fresh = _exports(S)
    for b in ("morton", "default", "morton", "sah"):
        morton(S, b)
        assert host_device.scene_build_info(S.scene)["builder"] == (2 if b == "morton" else 0)
        if b != "morton":
            for x, y in zip(_exports(S), fresh):
                assert np.array_equal(x, y)
    monkeypatch.setenv("YRT_BUILDER", "morton")
    assert host_device.scene_build_info(morton(S, "default").scene)["builder"] == 2
    assert host_device.scene_build_info(ts.exact_scene(host_device).scene)["builder"] == 2


def test_refit_poses_on_morton_trees(host_device):
    """ts.REFIT_POSES (a grid out of the bounds, three meshes at once, 558 point triangles, -3e5)
    on the host, where every commit rebuilds: each state's morton tree passes the checks."""
    S = morton(ts.refit_scene(host_device))
    for pose in ts.REFIT_POSES:
        pose(S)
        assert host_device.scene_build_info(S.scene)["builder"] == 2
        _check_state(S)
        check_structure(S)


@pytest.mark.parametrize("name", ["refit", "exact", "chain"])
def test_hits_through_the_morton_tree(host_device, name):
    """The kernel-order traversal of the exported morton tree finds brute force's hits (ids, and
    t, u, v bitwise) and occlusion flags, and never holds more stack entries than bvhDepth."""
    S = morton(SCENES[name](host_device))
    if name == "refit":
        org, dr, cut = ts.refit_rays(S, S.tri9[:782], S.tri9[:782], 4096)
    elif name == "chain":
        org, dr, _ = ts.chain_rays(S.tri9, 2048)
        cut = dr
    else:
        org, dr = ts.exact_rays()[:2]
        cut = dr
    nodes, tris, q = _exports(S)
    tb = S.info["triRecordBytes"]
    ref_hit, _ = ts.brute_force(S.tri9, S.flags, org, dr)
    _, hit = visits(S, org, dr)
    assert np.array_equal(ts.ids(hit), ts.ids(ref_hit))
    m = ts.ids(ref_hit) >= 0
    assert m.any() and np.array_equal(ts.bits(hit[m, :3]), ts.bits(ref_hit[m, :3]))
    _, ref_occ = ts.brute_force(S.tri9, S.flags, org, cut)
    h, _, _, occ = oracle.traverse_stats(q, tris, org, cut, any_hit=True, tri_bytes=tb)
    assert np.array_equal(ts.ids(occ) >= 0, ref_occ != 0)
    height = oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)[0]
    print(name, "stack height", int(height.max()), "bvhDepth", S.info["bvhDepth"])
    assert max(int(height.max()), int(h.max())) <= S.info["bvhDepth"]


def test_fallbacks(host_device):
    """One triangle: fallback 1. A NaN vertex: fallback 2 and the default builder's exports. The
    staircase: fallback 3 (its morton tree's stack bound is 87), a valid tree within the stack."""
    one = morton(soup_scene(host_device, 1))
    bi = host_device.scene_build_info(one.scene)
    assert (bi["builder"], bi["fallback"]) == (0, 1) and one.info["numNodes"] == 1
    S = nan_scene(host_device)
    default = _exports(S)
    bi = host_device.scene_build_info(morton(S).scene)
    assert (bi["builder"], bi["fallback"]) == (0, 2), bi
    for a, b in zip(_exports(S), default):
        assert np.array_equal(a, b)
    S = morton(staircase_scene(host_device))
    bi = host_device.scene_build_info(S.scene)
    assert (bi["builder"], bi["fallback"]) == (0, 3), bi
    k = np.sort(np_keys(S.tri9))
    assert (k[:4096] == 0).all() and np.array_equal(k[4096:4159], np.uint64(1) << np.arange(63, dtype=np.uint64))
    assert _check_state(S) == 0
    assert S.info["bvhDepth"] <= 63


def _inner(children, ni):
    """The node indices of node ni's inner children, in slot order."""
    c = children[ni][children[ni] != -1]
    return [int(x) >> 5 for x in c if x & 31 == 0]


@pytest.mark.parametrize("name", ["refit", "soup257"])
def test_node_numbering_of_both_builders(host_device, name):
    """Both builders write their nodes through one writer (common/yrt_bvh4.h) and number them
    themselves. Default builder: depth-first pre-order, node 0 the root; the walk from the root that
    visits a node's inner children in slot order meets the nodes as 0, 1, 2, ... "morton":
    breadth-first; the inner children of a level's nodes, in node and then slot order, are the
    consecutive indices after the level. Both: an empty slot is child -1 with lo = +inf, hi = -inf
    on every axis; the pad is 0. No tolerance."""
    S = SCENES[name](host_device)
    trees = {}
    for b in ("default", "morton"):
        morton(S, b)
        assert host_device.scene_build_info(S.scene)["builder"] == (2 if b == "morton" else 0)
        planes, children, pad = rr.split_nodes(_exports(S)[0])
        assert len(children) == S.info["numNodes"] > 4
        empty = children == -1
        assert empty.any() and not empty[0, :2].any()
        lo, hi = planes[:, 0::2, :], planes[:, 1::2, :]          # (node, axis, child)
        assert (lo.transpose(0, 2, 1)[empty] == np.inf).all() and (hi.transpose(0, 2, 1)[empty] == -np.inf).all()
        assert np.isfinite(lo.transpose(0, 2, 1)[~empty]).all() and np.isfinite(hi.transpose(0, 2, 1)[~empty]).all()
        assert not pad.any()
        trees[b] = children
    # depth-first pre-order
    children = trees["default"]
    order, stack = [], [0]
    while stack:
        ni = stack.pop()
        order.append(ni)
        stack += reversed(_inner(children, ni))
    assert order == list(range(len(children)))
    # breadth-first
    children = trees["morton"]
    level, after = [0], 1
    while level:
        nxt = [c for ni in level for c in _inner(children, ni)]
        assert nxt == list(range(after, after + len(nxt))), (level[:4], nxt[:8], after)
        level, after = nxt, after + len(nxt)
    assert after == len(children)
    assert any(len(_inner(children, ni)) > 1 for ni in range(len(children))), "no node with two inner children"


# measured ratios morton / SAH (the module docstring has the figures), plus 10 %: the inputs are
# deterministic; the margin keeps a later leaf-size change from tripping on the last digit
QUALITY = {"refit": (3.809 * 1.1, 1.416 * 1.1), "C3": (1.734 * 1.1, 1.005 * 1.1)}


@pytest.mark.parametrize("which", ["refit", "C3"])
def test_quality_against_the_sah_builder(host_device, which):
    """sahCost and the mean node visits of 4096 rays (oracle.count_visits, quantized nodes) of the
    morton tree, relative to the host SAH builder's: printed, and below the measured ratios + 10 %."""
    d = host_device
    if which == "refit":
        S = ts.refit_scene(d)
        org, dr, _ = ts.refit_rays(S, S.tri9[:782], S.tri9[:782], 4096)
        rows = {}
        for b in ("default", "morton"):
            morton(S, b)
            rows[b] = (d.scene_build_info(S.scene)["sahCost"], visits(S, org, dr)[0], S.info["numNodes"],
                       S.info["bvhDepth"])
    else:
        import yrt
        from helpers import c3_args
        from test_cpu_host import _incoherent
        rows = {}
        for b in ("default", "morton"):
            s = yrt.Session(c3_args(32, 1) + ["-builder", b], device=d)
            scene = s.info()["scene"]
            info = d.scene_info(scene)
            org, dr = _incoherent(s.export_frame(), 4096)
            nodes, tris = d.export_bvh(scene)
            nv, _, hit = oracle.count_visits(nodes, tris, org, dr, tri_bytes=info["triRecordBytes"],
                                             qnodes=d.export_qbvh(scene))
            bi = d.scene_build_info(scene)
            assert bi["builder"] == (2 if b == "morton" else 0) and bi["fallback"] == 0
            rows[b] = (bi["sahCost"], nv / len(org), info["numNodes"], info["bvhDepth"], ts.ids(hit).copy())
            s.close()
        assert np.array_equal(rows["default"][4], rows["morton"][4]), "hits differ between the builders"
    for b, r in rows.items():
        print(f"{which} {b}: sahCost {r[0]:.4f} node visits/ray {r[1]:.2f} nodes {r[2]} bvhDepth {r[3]}")
    sah, vis = rows["morton"][0] / rows["default"][0], rows["morton"][1] / rows["default"][1]
    print(f"{which} morton / SAH: sahCost {sah:.3f} node visits {vis:.3f}")
    assert sah < QUALITY[which][0] and vis < QUALITY[which][1]


# ============================================================================= GPU
_host_exports = {}


def host_exports(host_device, name, make):
    """The host loop's three exports of a scene, built once per session."""
    if name not in _host_exports:
        _host_exports[name] = _exports(morton(make(host_device)))
    return _host_exports[name]


GPU_SCENES = {"refit": ts.refit_scene, "exact": ts.exact_scene}
GPU_SCENES.update({f"soup{n}": SCENES[f"soup{n}"] for n in (2, 5, 64, 65)})


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_SCENES))
def test_gpu_tree_is_the_host_loops(gpu_device, host_device, name):
    """GPU test 1: the kernels' nodes, leaf records and quantized nodes equal the host loop's byte
    for byte, twice in a row; builder 1; the tree passes _check_state."""
    want = host_exports(host_device, name, GPU_SCENES[name])
    S = morton(GPU_SCENES[name](gpu_device))
    bi = gpu_device.scene_build_info(S.scene)
    assert (bi["builder"], bi["fallback"]) == (1, 0), bi
    first = _exports(S)
    for got, ref, what in zip(first, want, ("nodes", "leaf records", "quantized nodes")):
        assert len(got) == len(ref), (what, len(got), len(ref))
        assert np.array_equal(got, ref), (what, np.flatnonzero(got != ref)[:8])
    assert _check_state(S) == 0
    check_structure(S)
    S2 = morton(GPU_SCENES[name](gpu_device))
    for a, b in zip(_exports(S2), first):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_tree_of_a_large_mesh(gpu_device, host_device):
    """GPU test 2: 2^17 + 37 triangles: the exports equal the host loop's, every id appears once
    and the keys are ordered along the leaves; kernel timing reports the build kernels' time."""
    pos, idx = big_field()
    assert len(idx) == (1 << 17) + 37
    H = morton(ts.MeshScene(host_device, [(pos, idx, False)]))
    gpu_device.set_kernel_timing(True)
    try:
        S = morton(ts.MeshScene(gpu_device, [(pos, idx, False)]))
    finally:
        gpu_device.set_kernel_timing(False)
    bi = gpu_device.scene_build_info(S.scene)
    print("2^17 + 37 triangles:", bi, "host loop:", host_device.scene_build_info(H.scene))
    assert (bi["builder"], bi["fallback"]) == (1, 0) and 0 < bi["msKernels"] <= bi["msBuild"]
    assert bi["sahCost"] == host_device.scene_build_info(H.scene)["sahCost"]
    for got, ref in zip(_exports(S), _exports(H)):
        assert np.array_equal(got, ref)
    assert S.info["bvhDepth"] == H.info["bvhDepth"] <= 63
    gid = rr.split_tris(_exports(S)[1], S.info["triRecordBytes"])[3][:, 0]
    assert np.array_equal(np.sort(gid), np.arange(len(idx)))
    k = np_keys(S.tri9)[gid]
    assert (k[1:] >= k[:-1]).all()
    same = k[1:] == k[:-1]
    assert (gid[1:][same] > gid[:-1][same]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refit", "exact"])
def test_gpu_queries_on_morton_trees(gpu_device, name):
    """GPU test 3: yrtIntersect / yrtOccluded on the morton tree, 65 and 8191 rays, tfar infinite
    and half of the rays cut short: ids and flags equal brute force, t, u, v bitwise."""
    S = morton(GPU_SCENES[name](gpu_device))
    assert gpu_device.scene_build_info(S.scene)["builder"] == 1
    if name == "refit":
        org, dr, cut = ts.refit_rays(S, S.tri9[:782], S.tri9[:782], 8191)
    else:
        rng = np.random.default_rng(29)
        n = 8191
        org = np.zeros((n, 4), F)
        dr = np.zeros((n, 4), F)
        # a quarter-unit lattice of origins under and over the quads and the grid, straight up or
        # down: edges, vertices and the coincident copies are hit exactly
        org[:, 0] = rng.integers(-4, 160, n) * 0.25
        org[:, 1] = rng.integers(-4, 32, n) * 0.25
        up = np.arange(n) % 2 == 0
        org[:, 2] = np.where(up, 0.0, 2.0)
        dr[:, 2] = np.where(up, 1.0, -1.0)
        dr[:, 3] = np.inf
        cut = dr.copy()
        cut[(np.arange(n) // 2) % 2 == 0, 3] = 0.75
    for d in (dr, cut):
        ref_hit, ref_occ = ts.brute_force(S.tri9, S.flags, org, d)
        if d is dr:
            assert (ts.ids(ref_hit) >= 0).mean() > 0.05
        for n in (65, 8191):
            h, c = ts.query(gpu_device, S.scene, org, d, n=n)
            ts.compare(h, c, ref_hit[:n], ref_occ[:n])


def _frames(dev, S, size=48):
    """The 4 spp, depth-3 path-traced frame of S with each builder, and the oracle's."""
    imgs = {}
    for b in ("default", "morton"):
        morton(S, b)
        assert dev.scene_build_info(S.scene)["builder"] == (1 if b == "morton" else 0)
        r, blob = S.frame("pathtracer", spp=4, depth=3)
        imgs[b] = S.render(r, size)
    return imgs, oracle.render(blob, size, size, 1.0)[0]


@pytest.mark.gpu
def test_gpu_frames_do_not_depend_on_the_builder(gpu_device):
    """GPU test 4: the 48 x 48, 4 spp, depth-3 frame of refit_scene (pose a, the grid in view) is
    bit-identical between the builders and meets the oracle."""
    from helpers import parity
    S = ts.refit_scene(gpu_device)
    ts.refit_pose_a(S)
    imgs, ref = _frames(gpu_device, S)
    assert len(np.unique(imgs["morton"].reshape(-1, 3), axis=0)) > 48
    assert np.array_equal(imgs["morton"], imgs["default"]), np.argwhere(imgs["morton"] != imgs["default"])[:5]
    parity(imgs["morton"], ref, 0.999)


@pytest.mark.gpu
def test_gpu_frames_of_a_moving_mesh(gpu_device):
    """GPU test 4, moving geometry (the sphere with dPdt of tests/test_motion.py): the boxes span
    the frame time under both builders; frames bit-identical, and the oracle's."""
    from helpers import parity
    from test_cpu_host import yrt_lookat
    d = gpu_device
    sph = d.rtNewShape("sphere")
    d.rtSetFloat3(sph, "P", 0.0, 0.0, 0.0)
    d.rtSetFloat1(sph, "r", 1.0)
    d.rtSetInt1(sph, "numTheta", 16)
    d.rtSetInt1(sph, "numPhi", 32)
    d.rtSetFloat3(sph, "dPdt", 0.6, 0.0, 0.0)
    d.rtCommit(sph)
    mat = d.rtNewMaterial("Matte")
    d.rtSetFloat3(mat, "reflectance", 0.7, 0.5, 0.3)
    d.rtCommit(mat)
    amb = d.rtNewLight("ambientlight")
    d.rtSetFloat3(amb, "L", 1.0, 1.0, 1.0)
    d.rtCommit(amb)
    cam = d.rtNewCamera("pinhole")
    d.rtSetTransform(cam, "local2world", yrt_lookat((0, 0, -4), (0, 0, 0), (0, 1, 0)))
    d.rtSetFloat1(cam, "angle", 50.0)
    d.rtSetFloat1(cam, "aspectRatio", 1.0)
    d.rtCommit(cam)
    r = d.rtNewRenderer("pathtracer")
    d.rtSetInt1(r, "maxDepth", 3)
    d.rtSetInt1(r, "sampler.spp", 4)
    d.rtCommit(r)
    tm = d.rtNewToneMapper("default")
    d.rtCommit(tm)
    fb = d.rtNewFrameBuffer("RGB_FLOAT32", 48, 48)
    scene = d.rtNewScene("default")
    d.rtSetPrimitive(scene, 0, d.rtNewShapePrimitive(sph, mat))
    d.rtSetPrimitive(scene, 1, d.rtNewLightPrimitive(amb))
    imgs = {}
    for b in ("default", "morton"):
        d.rtSetString(scene, "builder", b)
        d.rtCommit(scene)
        bi = d.scene_build_info(scene)
        assert (bi["builder"], bi["fallback"]) == ((1, 0) if b == "morton" else (0, 0)), bi
        d.rtRenderFrame(r, cam, scene, tm, fb, 0)
        imgs[b] = d.framebuffer_array(fb, 48, 48, "RGB_FLOAT32").copy()
    ref, _ = oracle.render(d.export_frame(r, cam, scene), 48, 48, 1.0)
    assert len(np.unique(imgs["morton"].reshape(-1, 3), axis=0)) > 48
    assert np.array_equal(imgs["morton"], imgs["default"])
    parity(imgs["morton"], ref, 0.999)


@pytest.mark.gpu
def test_gpu_refit_after_a_morton_build(gpu_device):
    """GPU test 5: vertex-only commits after a morton build refit (the poses, and a round trip
    that returns the fresh exports); asking for "default" again rebuilds: no refit counted, the
    exports of a default build of the same triangles."""
    S = morton(ts.refit_scene(gpu_device))
    fresh = _exports(S)
    home = S.meshes[ts.R_GRID]["pos"].copy()
    ts.refit_pose_a(S)
    assert gpu_device.scene_refits(S.scene) == 1
    assert not np.array_equal(_exports(S)[0], fresh[0])
    S.move(ts.R_GRID, home)
    assert gpu_device.scene_refits(S.scene) == 2
    for a, b in zip(_exports(S), fresh):
        assert np.array_equal(a, b)
    S = morton(ts.refit_scene(gpu_device))
    _refit_all_poses(S)
    assert gpu_device.scene_build_info(S.scene)["builder"] == 1
    morton(S, "default")
    assert gpu_device.scene_refits(S.scene) == 0
    assert gpu_device.scene_build_info(S.scene)["builder"] == 0
    gpu_device.set_refit_commits(False)
    try:
        D = ts.refit_scene(gpu_device)
        for pose in ts.REFIT_POSES:
            pose(D)
        assert gpu_device.scene_refits(D.scene) == 0
    finally:
        gpu_device.set_refit_commits(True)
    for a, b in zip(_exports(S), _exports(D)):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_fallbacks(gpu_device):
    """GPU test 6: the staircase (fallback 3) and the NaN vertex (fallback 2) on the GPU: the same
    codes as the host loop's, valid trees from the host SAH builder."""
    S = morton(staircase_scene(gpu_device))
    bi = gpu_device.scene_build_info(S.scene)
    assert (bi["builder"], bi["fallback"]) == (0, 3), bi
    assert _check_state(S) == 0 and S.info["bvhDepth"] <= 63
    S = nan_scene(gpu_device)
    default = _exports(S)
    bi = gpu_device.scene_build_info(morton(S).scene)
    assert (bi["builder"], bi["fallback"]) == (0, 2), bi
    for a, b in zip(_exports(S), default):
        assert np.array_equal(a, b)
    one = morton(soup_scene(gpu_device, 1))
    bi = gpu_device.scene_build_info(one.scene)
    assert (bi["builder"], bi["fallback"]) == (0, 1), bi
