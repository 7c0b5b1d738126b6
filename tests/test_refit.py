"""The GPU BVH refit (refit_gpu_scene: k_refit_tris, k_refit_nodes level by level,
k_quantize_nodes) against a from-scratch reference (tests/refit_ref.py): after a commit that only
moves vertices, the exported leaf records, float boxes and quantized nodes are what the vertices
and the unchanged topology determine, bit for bit; no tolerance is involved anywhere.

The scene (trace_scenes.refit_meshes) has grids whose triangle counts are no multiple of 64,
slivers, and meshes of all-zero, huge, tiny, collapsed and negative coordinates; the poses move a
grid out of the built bounds (a), three meshes in one commit (b), a grid into one point (c) and a
grid to -3e5 (d). The CPU tests pin the reference itself on the host builder's trees.

Measured on the CPU (host builder): 1405 triangles; without spatial splits 1405 references, 326
nodes, bvhDepth 22; with YRT_SBVH=1 1627 references (222 duplicate leaf slots), 424 nodes,
bvhDepth 27. Of the 8191 query rays 99 % of those aimed at the moved grid hit it, 2 % of those
aimed at its old place hit anything, 39 % of the incoherent ones hit.
Measured on the MI355X: every record, box and quantized byte equalled the reference after each of
the four refits, with and without spatial splits, on the first run; t, u, v of the queries were
bitwise equal to brute force. Before refit_gpu_scene kept GpuScene::bboxLo / bboxHi up to date,
test_scene_bounds_follow_a_refit failed (bboxLo z -343.2 of the build against -742.5).
"""
import numpy as np
import pytest

import oracle
import refit_ref as rr
import trace_scenes as ts
from test_cpu_host import _qnode_planes


# ----------------------------------------------------------------------------- the checks
def _exports(S):
    nodes, tris = S.dev.export_bvh(S.scene)
    return nodes, tris, S.dev.export_qbvh(S.scene)


def _topology(S):
    """What a refit must leave alone: (child words, padding, the three .w words per leaf slot)."""
    nodes, tris, _ = _exports(S)
    _, children, pad = rr.split_nodes(nodes)
    return children, pad, rr.split_tris(tris, S.info["triRecordBytes"])[3]


def _check_state(S, before=None, unions=True):
    """The exported tree against the reference on S.tri9. before: _topology() of an earlier state
    that must be unchanged. unions=False (a fresh build with spatial splits, whose boxes are
    clipped): the boxes only lie inside the unions."""
    nodes, tris, q = _exports(S)
    planes, children, pad = rr.split_nodes(nodes)
    v0, e1, e2, w = rr.split_tris(tris, S.info["triRecordBytes"])
    gid = w[:, 0]
    assert len(gid) == S.info["numTriRefs"] and len(children) == S.info["numNodes"]
    assert np.array_equal(np.unique(gid), np.arange(len(S.tri9))), "every triangle in some leaf"
    if before is not None:
        assert np.array_equal(children, before[0]) and np.array_equal(pad, before[1]), "topology: nodes"
        assert np.array_equal(w, before[2]), "topology: leaf order, .w words"
    assert np.array_equal(w[:, 1].view(np.uint32), S.flags[gid])
    # leaf records, duplicates included
    for got, want, name in zip((v0, e1, e2), rr.leaf_records(S.tri9, gid), ("v0", "e1", "e2")):
        bad = np.flatnonzero((ts.bits(got) != ts.bits(want)).any(1))
        assert len(bad) == 0, (name, len(bad), bad[:8], gid[bad[:8]])
    # float boxes
    want, valid = rr.union_boxes(children, gid, S.tri9)
    v = np.broadcast_to(valid[:, None, :], planes.shape)
    if unions:
        bad = np.argwhere((ts.bits(planes) != ts.bits(want)) & v)
        assert len(bad) == 0, ("boxes", len(bad), bad[:8])
    else:
        assert (planes[:, 0::2][v[:, 0::2]] >= want[:, 0::2][v[:, 0::2]]).all()
        assert (planes[:, 1::2][v[:, 1::2]] <= want[:, 1::2][v[:, 1::2]]).all()
    # quantized nodes: the quantizer's bytes of the exported float nodes
    wq = rr.quantize(planes, children).reshape(-1, 64)
    bad = np.flatnonzero((q.reshape(-1, 64) != wq).any(1))
    assert len(bad) == 0, ("quantized", len(bad), bad[:8], q.reshape(-1, 64)[bad[:2]], wq[bad[:2]])
    # containment by one quantum
    lo, hi, scale, qchild = _qnode_planes(q)
    assert np.array_equal(qchild, children)
    P = planes.astype(np.float64)
    for a in range(3):
        s_ = scale[:, a][:, None]
        assert np.all((lo[:, a, :] <= P[:, 2 * a, :] - s_) | ~valid)
        assert np.all((hi[:, a, :] >= P[:, 2 * a + 1, :] + s_) | ~valid)
    return len(gid) - len(S.tri9)


def _bounds(S):
    v = S.tri9.reshape(-1, 3)
    return v.min(0), v.max(0)


# ============================================================================= CPU
def test_reference_equals_the_host_builder(host_device):
    """Without spatial splits the builder's records, boxes and quantized bytes are the
    reference's, exactly; the scene has the sizes the GPU tests rely on."""
    S = ts.refit_scene(host_device)
    assert [len(m["idx"]) for m in S.meshes[:4]] == [782, 558, 2, 40]
    assert S.info["numTriangles"] == 1405 == S.info["numTriRefs"]
    assert _check_state(S) == 0
    print("sah: nodes", S.info["numNodes"], "refs", S.info["numTriRefs"], "depth", S.info["bvhDepth"])
    assert S.info["bvhDepth"] <= 63


def test_reference_with_spatial_splits(host_device, monkeypatch):
    """YRT_SBVH=1: the quantized bytes are the reference's; the builder's clipped boxes lie inside
    the whole-triangle unions; at least 100 duplicate leaf slots (the GPU test's precondition)."""
    monkeypatch.setenv("YRT_SBVH", "1")
    S = ts.refit_scene(host_device)
    dup = _check_state(S, unions=False)
    print("sbvh: nodes", S.info["numNodes"], "refs", S.info["numTriRefs"], "depth", S.info["bvhDepth"])
    assert dup == S.info["numTriRefs"] - S.info["numTriangles"] >= 100
    assert S.info["bvhDepth"] <= 63
    planes, children, _ = rr.split_nodes(_exports(S)[0])
    want, valid = rr.union_boxes(children, _topology(S)[2][:, 0], S.tri9)
    assert (ts.bits(planes) != ts.bits(want))[np.broadcast_to(valid[:, None, :], planes.shape)].any(), "no box clipped"


def test_the_check_notices_one_wrong_word(host_device, monkeypatch):
    """_check_state on tampered exports of the spatial-split tree: a duplicate leaf slot left one
    ulp off, a box plane one ulp too small, a plane byte rounded inward by one quantum and a
    changed child word each fail it."""
    from types import SimpleNamespace
    S0 = ts.refit_scene(host_device)
    nodes0, tris0, q0 = _exports(S0)
    monkeypatch.setenv("YRT_SBVH", "1")
    S = ts.refit_scene(host_device)
    nodes, tris, q = _exports(S)
    gid = rr.split_tris(tris)[3][:, 0]
    dup = np.flatnonzero(np.bincount(gid) > 1)[0]
    slot = np.flatnonzero(gid == dup)[-1]

    def tampered(nodes=nodes, tris=tris, q=q, info=S.info):
        dev = SimpleNamespace(export_bvh=lambda s: (nodes, tris), export_qbvh=lambda s: q)
        return SimpleNamespace(dev=dev, scene=None, info=info, tri9=S.tri9, flags=S.flags)

    _check_state(tampered(), unions=False)
    t = tris.copy()
    t.view(np.uint32)[12 * slot] += 1                    # v0.x of the last duplicate
    with pytest.raises(AssertionError, match="v0"):
        _check_state(tampered(tris=t), unions=False)
    n = nodes0.copy()
    w = n.view(np.float32).reshape(-1, 32)
    w[0, 0] = np.nextafter(w[0, 0], np.float32(np.inf))  # lox of the root's first child, tree without splits
    _check_state(tampered(nodes0, tris0, q0, S0.info))
    with pytest.raises(AssertionError, match="boxes"):
        _check_state(tampered(n, tris0, q0, S0.info))
    qq = q.copy()
    qq.reshape(-1, 64)[0, 32] += 1                       # its lo x byte
    with pytest.raises(AssertionError, match="quantized"):
        _check_state(tampered(q=qq), unions=False)
    n = nodes.copy()
    c = n.view(np.int32).reshape(-1, 32)
    c[0, 24], c[0, 25] = c[0, 25], c[0, 24]              # the root's first two child words swapped
    with pytest.raises(AssertionError, match="topology"):
        _check_state(tampered(nodes=n), before=_topology(S), unions=False)


def test_poses_on_the_host(host_device):
    """The poses do what the GPU tests need of them (the host device rebuilds on every commit, so
    each state is a fresh tree): (a) leaves the built bounds, (b) moves three meshes, (c) makes
    558 point triangles, (d) reaches -3e5; MeshScene.move keeps tri9 the scene's triangles."""
    S = ts.refit_scene(host_device)
    lo0, hi0 = _bounds(S)
    assert np.array_equal(S.info["bboxLo"], lo0) and np.array_equal(S.info["bboxHi"], hi0)
    old = S.tri9.copy()
    for pose in ts.REFIT_POSES:
        before = S.tri9.copy()
        pose(S)
        assert np.array_equal(oracle.scene_triangles(S.blob), S.tri9)
        assert not np.signbit(S.tri9[S.tri9 == 0]).any()
        _check_state(S)
        moved = (S.tri9 != before).any(1)
        if pose is ts.refit_pose_a:
            assert moved[:782].all() and not moved[782:].any()
            assert _bounds(S)[1][1] > hi0[1] + 10 and _bounds(S)[0][2] < lo0[2] - 10
        elif pose is ts.refit_pose_b:
            assert moved[782:1382].all() and not moved[:782].any() and not moved[1382:].any()
        elif pose is ts.refit_pose_c:
            assert (S.tri9[782:1340] == np.tile(S.tri9[782, :3], 3)).all()
        else:
            assert moved[:782].all() and S.tri9[:782].max() < -2.9e5
    assert (old[1382:] == S.tri9[1382:]).all()


def test_refit_rays_reach_their_targets(host_device):
    """The query test's rays, on the host: brute force equals the oracle; the rays aimed at the
    moved grid mostly hit it, the rays at its old place mostly hit something else or nothing, and
    the cut rays lose some of the hits."""
    S = ts.refit_scene(host_device)
    old9 = S.tri9[:782].copy()
    ts.refit_pose_a(S)
    org, dr, cut = ts.refit_rays(S, old9, S.tri9[:782], 8191)
    bh, bo = ts.brute_force(S.tri9, S.flags, org, dr)
    ref = oracle.trace(S.blob, org, dr)
    assert np.array_equal(ts.ids(bh), ts.ids(ref))
    m = ts.ids(bh) >= 0
    assert np.array_equal(ts.bits(bh[m, :3]), ts.bits(ref[m, :3]))
    kind = np.arange(len(org)) % 3
    on_grid = (ts.ids(bh) >= 0) & (ts.ids(bh) < 782)
    print("hits by kind:", [float(m[kind == k].mean()) for k in range(3)], "on the grid:",
          [float(on_grid[kind == k].mean()) for k in range(3)])
    assert on_grid[kind == 0].mean() > 0.8 and on_grid[kind == 1].mean() < 0.05
    ch, co = ts.brute_force(S.tri9, S.flags, org, cut)
    assert np.array_equal(co, ts.ids(oracle.trace(S.blob, org, cut, any_hit=True)))
    assert 0.1 * bo.sum() < co.sum() < 0.9 * bo.sum()


# ============================================================================= GPU
def _refit_all_poses(S):
    """Poses (a) to (d) in separate commits; after each the topology is the build's, the state the
    reference's and the counter one higher."""
    before = _topology(S)
    for k, pose in enumerate(ts.REFIT_POSES):
        pose(S)
        assert S.dev.scene_refits(S.scene) == k + 1, pose.__name__
        _check_state(S, before)


@pytest.mark.gpu
def test_state_after_each_pose(gpu_device):
    """Test 1: leaf order, child words and .w words unchanged; every record, box and quantized
    byte equal to the reference; containment by one quantum."""
    S = ts.refit_scene(gpu_device)
    assert S.info["numTriRefs"] == S.info["numTriangles"] == 1405
    _check_state(S)
    _refit_all_poses(S)


@pytest.mark.gpu
def test_state_with_spatial_splits(gpu_device, monkeypatch):
    """Test 3: with YRT_SBVH=1 at least 100 leaf slots are duplicates; after each pose every one
    of them carries the new vertices, and the boxes, clipped by the builder, are the
    whole-triangle unions."""
    monkeypatch.setenv("YRT_SBVH", "1")
    S = ts.refit_scene(gpu_device)
    assert _check_state(S, unions=False) >= 100
    _refit_all_poses(S)


@pytest.mark.gpu
def test_round_trip(gpu_device):
    """Test 2: a mesh moved away and back in two commits leaves the three exports byte-identical
    to the fresh build's, with two refits counted; commits that move nothing (the same slots, or
    the same vertices in a new mesh) change neither the counter nor the exports."""
    S = ts.refit_scene(gpu_device)
    fresh = _exports(S)
    home = S.meshes[ts.R_GRID]["pos"].copy()
    ts.refit_pose_a(S)
    away = _exports(S)
    assert not np.array_equal(away[0], fresh[0]) and not np.array_equal(away[1], fresh[1])
    assert not np.array_equal(away[2], fresh[2])
    S.move(ts.R_GRID, home)
    assert gpu_device.scene_refits(S.scene) == 2
    for a, b in zip(_exports(S), fresh):
        assert np.array_equal(a, b)
    S.commit()
    S.move(ts.R_GRID2, S.meshes[ts.R_GRID2]["pos"].copy())
    assert gpu_device.scene_refits(S.scene) == 2
    for a, b in zip(_exports(S), fresh):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("sbvh", ["0", "1"], ids=["sah", "sbvh"])
def test_queries_on_the_refit_tree(gpu_device, monkeypatch, sbvh):
    """Test 4: yrtIntersect / yrtOccluded on the tree refit to pose (a), 65 and 8191 rays (a third
    at the grid's new place, a third at its old place, a third from inside the new bounds), with
    tfar infinite and with half of the rays cut short: ids and flags equal brute force on the new
    triangles, t, u, v bitwise."""
    monkeypatch.setenv("YRT_SBVH", sbvh)
    S = ts.refit_scene(gpu_device)
    old9 = S.tri9[:782].copy()
    ts.refit_pose_a(S)
    assert gpu_device.scene_refits(S.scene) == 1
    org, dr, cut = ts.refit_rays(S, old9, S.tri9[:782], 8191)
    for d in (dr, cut):
        ref_hit, ref_occ = ts.brute_force(S.tri9, S.flags, org, d)
        assert (ts.ids(ref_hit) >= 0).mean() > 0.3
        for n in (65, 8191):
            h, c = ts.query(gpu_device, S.scene, org, d, n=n)
            ts.compare(h, c, ref_hit[:n], ref_occ[:n])


@pytest.mark.gpu
def test_shading_records_after_a_refit(gpu_device):
    """Test 5: the grid's vertex normals turn with pose (a). The path-traced frame (48 x 48, 4 spp,
    depth 3, ambient light) of the refit scene equals the frame of the same commits with refits
    switched off (a rebuild), bit for bit, and the oracle's frame of the exported scene."""
    from helpers import parity
    imgs = {}
    try:
        for refit in (True, False):
            gpu_device.set_refit_commits(refit)
            S = ts.refit_scene(gpu_device)
            ts.refit_pose_a(S)
            assert gpu_device.scene_refits(S.scene) == (1 if refit else 0)
            r, blob = S.frame("pathtracer", spp=4, depth=3)
            imgs[refit] = S.render(r, 48)
            if refit:
                ref, _ = oracle.render(blob, 48, 48, 1.0)
    finally:
        gpu_device.set_refit_commits(True)
    assert len(np.unique(imgs[True].reshape(-1, 3), axis=0)) > 48   # the grid is in view, shaded
    assert np.array_equal(imgs[True], imgs[False]), np.argwhere(imgs[True] != imgs[False])[:5]
    parity(imgs[True], ref, 0.999)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["indices", "vertex count", "material"])
def test_refused_commits_rebuild(gpu_device, what):
    """Test 6: after one refit, a commit with another index list of the same size, another vertex
    count or another material rebuilds: the counter is back at 0 and the new tree is the
    reference's for the new triangles."""
    S = ts.refit_scene(gpu_device)
    ts.refit_pose_c(S)
    assert gpu_device.scene_refits(S.scene) == 1
    m = S.meshes[ts.R_GRID]
    if what == "indices":
        m["idx"] = np.ascontiguousarray(m["idx"][::-1, [1, 2, 0]])
        S.move(ts.R_GRID, m["pos"] + np.float32(0.5))
    elif what == "vertex count":
        S.move(ts.R_GRID, np.concatenate([m["pos"], [[1, 2, 3]]]).astype(np.float32),
               np.concatenate([m["nor"], [[0, 1, 0]]]).astype(np.float32))
    else:
        d = gpu_device
        mat = d.rtNewMaterial("Matte")
        d.rtSetFloat3(mat, "reflectance", 0.25, 0.5, 0.75)
        d.rtCommit(mat)
        S._set_mesh(ts.R_GRID, m["pos"] + np.float32(0.5), m["nor"], mat=mat)
        S.commit()
    assert gpu_device.scene_refits(S.scene) == 0
    _check_state(S)


@pytest.mark.gpu
def test_scene_bounds_follow_a_refit(gpu_device):
    """Test 7: scene_info's bboxLo / bboxHi are the bounds of the current vertices after a refit
    that leaves the built bounds, and after a second refit."""
    S = ts.refit_scene(gpu_device)
    lo0, hi0 = _bounds(S)
    assert np.array_equal(np.float32(S.info["bboxLo"]), lo0) and np.array_equal(np.float32(S.info["bboxHi"]), hi0)
    ts.refit_pose_a(S)
    assert gpu_device.scene_refits(S.scene) == 1
    lo, hi = _bounds(S)
    assert hi[1] > hi0[1] and lo[2] < lo0[2]
    assert np.array_equal(np.float32(S.info["bboxLo"]), lo) and np.array_equal(np.float32(S.info["bboxHi"]), hi)
    ts.refit_pose_c(S)
    lo, hi = _bounds(S)
    assert np.array_equal(np.float32(S.info["bboxLo"]), lo) and np.array_equal(np.float32(S.info["bboxHi"]), hi)
