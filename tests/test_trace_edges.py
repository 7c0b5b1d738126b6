"""The ray-query kernel (kernels/k_trace.h) where random rays never take it: the spill of its
16-entry LDS ring stack to global memory, lane refill with unaligned chunks, and the rules that
hold only on exact equality (ties, range edges, den == 0, zero direction components).
Everything here runs the static instantiations (MOTION = false); tests/test_trace_motion.py does
the same for the moving-geometry ones, through the timed calls.

References: a brute-force test of every ray against every triangle in numpy float32
(trace_scenes.brute_force, no BVH and so no box test of any kind), the oracle's own trace, and,
for the named cases of the exact scene, ids written by hand. The CPU tests show that the three
agree and that the rays reach the mechanism (stack heights from the oracle's simulation of the
kernel's traversal of the exported quantized nodes, tie winners that are not the first triangle
accepted); the GPU tests compare yrtIntersect / yrtOccluded with them bit for bit.

Measured on the CPU (the asserted lower bounds are the issue's, 2 * 16 + 2 = 34 entries):
  chain scene: bvhDepth 37, greatest stack height 36; 1024 of the 4096 rays reach height >= 34
  in closest-hit order and 1090 in any-hit order; 768 and 813 of them hit (the backstop
  triangle) through a stack entry that waited under 36 entries, so spilled and restored through
  two generations of the ring; all 4096 camera rays through the 64 x 64 pixel centres and all
  16384 captured depth-0 rays of the 4 spp frame reach height >= 34.
  exact scene: 113 rays whose winner is not the first triangle accepted.
u and v: the oracle divides U / |den| and V / |den| like the kernel, and brute force, oracle and
the simulation agree on t, u, v bit for bit on every scene. On the MI355X t, u and v of every
hit in every test below were bitwise equal to them as well; no tolerance is used.

Finding: the brute force disagreed with the oracle (and the float-node box test that k_pick /
k_debug had then shared the flaw) for rays along a box face, see test_oracle_ray_along_a_box_face
and test_pick_along_a_box_face; both box tests were fixed. The device has since dropped that box
test: k_pick, k_debug and k_guides walk the quantized nodes through closest_hit, with k_trace's
box test, and test_guides_equal_ray_queries compares the two kernels directly.
"""
import numpy as np
import pytest

import oracle
import trace_scenes as ts
from trace_scenes import bits as _bits, compare as _compare, ids as _ids, query as _query  # noqa: F401

RING = 16                # YRT_LDS_STACK*: entries of the LDS ring
DEEP = 2 * RING + 2      # a second spilled generation, plus the kernel's parked leaf and pop-ahead


def _references(S, org, dr):
    """(closest hits, occlusion flags): brute force, checked against the oracle bit for bit
    (t, u, v of hits, ids, flags)."""
    bh, bo = ts.brute_force(S.tri9, S.flags, org, dr)
    ref = oracle.trace(S.blob, org, dr)
    ref_occ = _ids(oracle.trace(S.blob, org, dr, any_hit=True))
    assert np.array_equal(_ids(bh), _ids(ref)), np.flatnonzero(_ids(bh) != _ids(ref))[:8]
    m = _ids(bh) >= 0
    assert np.array_equal(_bits(bh[m, :3]), _bits(ref[m, :3]))
    assert np.array_equal(bo, ref_occ)
    return bh, bo


def _records_match(S):
    """The brute force's triangles (v0, e1 = v0 - v1, e2 = v2 - v0, cull flag by mesh) are the
    device's leaf records and the oracle's triangles, id for id."""
    v0, e1, e2, fl = S.leaf_records()
    t = S.tri9
    assert np.array_equal(oracle.scene_triangles(S.blob), t)
    assert np.array_equal(v0, t[:, 0:3]) and np.array_equal(e1, t[:, 0:3] - t[:, 3:6])
    assert np.array_equal(e2, t[:, 6:9] - t[:, 0:3]) and np.array_equal(fl, S.flags)


# ============================================================================= CPU
@pytest.fixture(scope="module")
def chain_cpu(host_device):
    S = ts.chain_scene(host_device)
    org, dr, kind = ts.chain_rays(S.tri9)
    return S, org, dr, kind


@pytest.fixture(scope="module")
def exact_cpu(host_device):
    return ts.exact_scene(host_device)


def test_chain_brute_force_equals_oracle(chain_cpu):
    S, org, dr, kind = chain_cpu
    _records_match(S)
    bh, bo = _references(S, org, dr)
    # the set mixes hits and misses in every wave of 64
    hit = (_ids(bh) >= 0).reshape(-1, 64)
    assert hit.any(1).all() and (~hit).any(1).all()


def test_chain_reaches_the_spill(chain_cpu):
    """bvhDepth >= 36 (and <= 63, the spill buffer's bound: spill index <= bvhDepth - 1 - 16 <
    YRT_SPILL_1 = 48); per the simulation on the quantized nodes at least 64 closest-hit and 64
    any-hit rays reach 34 entries, and at least 64 of each report a hit whose stack entry waited
    under 34 entries. Every wave of 64 holds deep and shallow rays."""
    S, org, dr, kind = chain_cpu
    assert 36 <= S.info["bvhDepth"] <= 63
    q, tris, tb = S.bvh()
    bh, bo = ts.brute_force(S.tri9, S.flags, org, dr)
    for any_hit in (False, True):
        h, _, under, hit = oracle.traverse_stats(q, tris, org, dr, any_hit=any_hit, tri_bytes=tb)
        print("any" if any_hit else "closest", "max height", h.max(), "rays >= 34:", int((h >= DEEP).sum()),
              "hits under >= 34:", int((under >= DEEP).sum()))
        assert h.max() <= S.info["bvhDepth"]
        assert (h >= DEEP).sum() >= 64
        assert (under >= DEEP).sum() >= 64
        per_wave = h.reshape(-1, 64)
        assert ((per_wave >= DEEP).any(1) & (per_wave <= RING - 3).any(1)).all()
        if any_hit:
            assert np.array_equal((_ids(hit) >= 0).astype(np.int32), bo)
        else:
            assert np.array_equal(_bits(hit), _bits(bh))
    # the deep hits are the backstop
    deep = (oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)[2] >= DEEP)
    assert (_ids(bh)[deep] == ts.CHAIN_WALL).all()


def test_chain_camera_rays_are_deep(chain_cpu):
    """The chain camera's rays through the 64 x 64 pixel centres: at least 64 reach 34 entries,
    and some hit chain triangles instead of the backstop (the frame is not one flat colour)."""
    S = chain_cpu[0]
    px = (np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).reshape(-1, 2) + 0.5) / 64.0
    o, d = oracle.camera_rays(S.blob, px)
    org = np.concatenate([o, np.zeros((len(o), 1), np.float32)], 1)
    dr = np.concatenate([d, np.full((len(d), 1), np.inf, np.float32)], 1)
    q, tris, tb = S.bvh()
    h, _, _, hit = oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)
    print("camera rays >= 34:", int((h >= DEEP).sum()), "max", h.max())
    assert (h >= DEEP).sum() >= 64
    ids = _ids(hit)
    assert ((ids >= 0) & (ids != ts.CHAIN_WALL)).sum() >= 64 and (ids == ts.CHAIN_WALL).sum() >= 64


def test_launch_chunks():
    """The launcher's constants (16384 blocks of one wave) give the long run chunks of 97 rays:
    unaligned, and a last wave with a partial chunk; the existing direct tests (65,536 and 4,096
    rays) have chunks of exactly 64 and never refill."""
    chunk, waves = ts.launch_chunk(ts.LONG_N)
    assert (chunk, waves) == (97, 16384)
    assert waves * 96 < ts.LONG_N <= waves * 97
    assert ts.LONG_N % chunk not in (0, 64) and chunk % 64 != 0
    assert ts.launch_chunk(1 << 16)[0] == 64 and ts.launch_chunk(4096)[0] == 64
    assert ts.launch_chunk(4097) == (64, 65) and ts.launch_chunk(1) == (64, 1) and ts.launch_chunk(0) == (64, 1)


def test_exact_cases_three_ways(exact_cpu):
    """Hand-written ids and distances, brute force and the oracle agree on every named case; the
    occlusion flag is 'some triangle accepted'. At least 32 rays have a winner that is not the
    first triangle the kernel's order accepts (measured: 113)."""
    S = exact_cpu
    _records_match(S)
    org, dr, want, want_t, names = ts.exact_rays()
    bh, bo = _references(S, org, dr)
    got = _ids(bh)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(names[i], int(want[i]), int(got[i])) for i in bad[:8]]
    m = want >= 0
    assert np.array_equal(bh[m, 0], want_t[m]), [names[i] for i in np.flatnonzero(m & (bh[:, 0] != want_t))[:8]]
    assert np.array_equal(bo, m.astype(np.int32))
    q, tris, tb = S.bvh()
    h, differs, _, hit = oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)
    assert np.array_equal(_bits(hit[m]), _bits(bh[m])) and np.array_equal(_ids(hit), got)
    print("winner is not the first accepted:", int(differs.sum()))
    assert differs.sum() >= 32
    occ = _ids(oracle.traverse_stats(q, tris, org, dr, any_hit=True, tri_bytes=tb)[3]) >= 0
    assert np.array_equal(occ.astype(np.int32), bo)


def test_exact_origins_on_node_planes(exact_cpu):
    """Origins exactly on a plane of the quantized nodes with a +0 / -0 direction component:
    brute force, the oracle and the simulated kernel traversal agree."""
    S = exact_cpu
    q, tris, tb = S.bvh()
    org, dr = ts.node_plane_rays(q, S.info["bboxLo"], S.info["bboxHi"])
    assert len(org) >= 64
    bh, bo = _references(S, org, dr)
    assert 0.1 < bo.mean() < 0.9
    hit = oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)[3]
    assert np.array_equal(_ids(hit), _ids(bh))
    m = _ids(bh) >= 0
    assert np.array_equal(_bits(hit[m]), _bits(bh[m]))


def test_oracle_ray_along_a_box_face(exact_cpu):
    """A ray whose zero direction component leaves it in the plane of a box face (x = 4, the edge
    of the 40 copies: 0 * 1e20 = 0 as the slab exit) still meets that box: the oracle's own BVH
    returns the smallest id, not whichever copy a wider box happened to hold (it returned 78)."""
    S = exact_cpu
    org = np.array([[4, 2, 0, 0], [4, 4, 0, 0], [0, 4, 0, 0], [2, 4, 2, 0]], np.float32)
    dr = np.array([[0, 0, 1, np.inf], [-0.0, 0, 1, np.inf], [0, -0.0, 1, np.inf], [0, 0, -1, np.inf]], np.float32)
    assert list(_ids(oracle.trace(S.blob, org, dr))) == [0, 0, 1, 1]


# ============================================================================= GPU
@pytest.fixture(scope="module")
def chain_gpu(gpu_device):
    S = ts.chain_scene(gpu_device)
    assert S.info["bvhDepth"] <= 63  # before any launch: the spill index stays below YRT_SPILL_1
    return S


@pytest.mark.gpu
def test_chain_queries_gpu(gpu_device, chain_gpu):
    """Spill: the 4096 chain rays (1024 at stack height 36 in either order, mixed per wave with
    shallow rays and hits) through yrtIntersect / yrtOccluded equal brute force and the oracle:
    ids and flags exact, t, u, v bitwise equal (measured on the MI355X: bitwise equal)."""
    S = chain_gpu
    org, dr, _ = ts.chain_rays(S.tri9)
    q, tris, tb = S.bvh()
    for any_hit in (False, True):
        h = oracle.traverse_stats(q, tris, org, dr, any_hit=any_hit, tri_bytes=tb)[0]
        assert (h >= DEEP).sum() >= 64  # the device's own tree is as deep as the host build's
    ref_hit, ref_occ = _references(S, org, dr)
    _compare(*_query(gpu_device, S.scene, org, dr), ref_hit, ref_occ)


@pytest.mark.gpu
def test_chain_debug_frame_and_pick(gpu_device, chain_gpu):
    """The same scene through closest_hit (quantized nodes, private 64-entry stack): a 64 x 64 debug
    frame is bit-exact against the oracle, and a pick along the axis returns the brute-force hit
    point on the backstop."""
    S = chain_gpu
    r, blob = S.frame("debug")
    img = S.render(r, 64)
    ref, _ = oracle.render(blob, 64, 64, 1.0)
    assert np.array_equal(img, ref), np.argwhere(img != ref)[:5]
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 8
    hit, p = gpu_device.rtPick(S.camera, 0.5, 0.5, S.scene)
    o, d = oracle.camera_rays(blob, [[0.5, 0.5]])
    org = np.array([[*o[0], 0.0]], np.float32)
    dr = np.array([[*d[0], np.inf]], np.float32)
    bh, _ = ts.brute_force(S.tri9, S.flags, org, dr)
    assert hit and _ids(bh)[0] == ts.CHAIN_WALL
    want = o[0] + bh[0, 0] * d[0]
    assert want.dtype == np.float32
    assert np.array_equal(np.array(p, np.float32), want), (p, want)


@pytest.mark.gpu
def test_chain_fused_primary(gpu_device, chain_gpu, monkeypatch):
    """The fused depth-0 kernel k_trace<false, false, 1> on the chain: 64 x 64 at 4 spp with
    YRT_PRIMARY=0 (k_raygen + queued trace) and 2 (fused) give identical frames and ray counts,
    both at parity with the oracle; of the captured depth-0 rays at least 64 reach 34 entries
    (measured: all 16384)."""
    S = chain_gpu
    d = gpu_device
    r, blob = S.frame("pathtracer", spp=4)
    d.set_ray_capture(1 << 15)
    try:
        S.render(r, 64)
        org, dr, total = d.captured_rays(False, 0)
    finally:
        d.set_ray_capture(0)
    assert total == 64 * 64 * 4 == len(org)
    q, tris, tb = S.bvh()
    h = oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)[0]
    print("captured depth-0 rays >= 34:", int((h >= DEEP).sum()))
    assert (h >= DEEP).sum() >= 64
    ref, _ = oracle.render(blob, 64, 64, 1.0)
    out = []
    for prim in ("0", "2"):
        monkeypatch.setenv("YRT_PRIMARY", prim)
        img = S.render(r, 64)
        st = d.render_stats()
        out.append((img, st["raysClosest"], st["raysShadow"]))
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:] and out[0][1] >= 64 * 64 * 4
    from helpers import parity
    for img, _, _ in out:
        parity(img, ref, 0.999)


@pytest.fixture(scope="module")
def refill_set(gpu_device):
    """C3, 65,536 incoherent rays with a quarter made cheap or void; the oracle's closest hits
    and occlusion flags, computed once."""
    import yrt
    from helpers import c3_args
    from test_gpu_parity import _rays
    s = yrt.Session(c3_args(64, 1) + ["-fb", "RGB_FLOAT32"], device=gpu_device)
    blob = s.export_frame()
    info = gpu_device.scene_info(s.info()["scene"])
    assert info["bvhDepth"] <= 63
    org, dr = ts.refill_base(*_rays(blob, 1 << 16), info["bboxLo"], info["bboxHi"])
    ref = oracle.trace(blob, org, dr)
    ref_occ = _ids(oracle.trace(blob, org, dr, any_hit=True))
    for a in (org, dr, ref, ref_occ):
        a.setflags(write=False)
    # the void kinds return nothing, the rest still hits mostly
    i = np.arange(len(org))
    void = (i % 4 == 1) & ((i // 4) % 4 < 3)
    assert (_ids(ref)[void] == -1).all() and (_ids(ref)[i % 4 != 1] >= 0).mean() > 0.5
    yield s.info()["scene"], org, dr, ref, ref_occ
    s.close()


@pytest.mark.gpu
def test_refill_long_run(gpu_device, refill_set):
    """Lane refill: 2^20 + 2^19 + 37 rays drawn from the base set give chunks of 97 rays per
    wave (test_launch_chunks): every wave refills, at unaligned offsets, and the last one ends in
    a partial chunk. Results equal ref[index]; every slot is written and the guard is not."""
    scene, org, dr, ref, ref_occ = refill_set
    idx = np.random.default_rng(3).integers(0, len(org), size=ts.LONG_N)
    h, c = _query(gpu_device, scene, org[idx], dr[idx])
    _compare(h, c, ref[idx], ref_occ[idx])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_refill_small_counts(gpu_device, refill_set, n):
    scene, org, dr, ref, ref_occ = refill_set
    h, c = _query(gpu_device, scene, org, dr, n=n)
    _compare(h, c, ref[:n], ref_occ[:n])


@pytest.mark.gpu
def test_zero_rays(gpu_device, refill_set):
    """n = 0 with valid one-element buffers: both calls succeed and write nothing (the kernel's
    one block reads the count, finds its chunk empty and returns before touching a ray)."""
    scene, org, dr, _, _ = refill_set
    h, c = _query(gpu_device, scene, org, dr, n=0, guard=1)
    assert len(h) == 0 and len(c) == 0


@pytest.mark.gpu
def test_exact_cases_gpu(gpu_device):
    """The exact-equality scene on the device: the hand-written cases and the origins on node
    planes equal brute force (ids, flags, and t, u, v bitwise; measured: bitwise equal)."""
    S = ts.exact_scene(gpu_device)
    assert S.info["bvhDepth"] <= 63
    org, dr, want, want_t, names = ts.exact_rays()
    q, tris, tb = S.bvh()
    assert oracle.traverse_stats(q, tris, org, dr, tri_bytes=tb)[1].sum() >= 32
    po, pd = ts.node_plane_rays(q, S.info["bboxLo"], S.info["bboxHi"])
    org, dr = np.concatenate([org, po]), np.concatenate([dr, pd])
    ref_hit, ref_occ = _references(S, org, dr)
    h, c = _query(gpu_device, S.scene, org, dr)
    bad = np.flatnonzero(_ids(h)[:len(want)] != want)
    assert len(bad) == 0, [(names[i], int(want[i]), int(_ids(h)[i])) for i in bad[:8]]
    _compare(h, c, ref_hit, ref_occ)


@pytest.mark.gpu
def test_pick_along_a_box_face(gpu_device):
    """closest_hit on a ray along a box face (float-node planes are the triangles' own coordinates,
    the quantized nodes' lie a quantum outside): the exact scene's camera looks up the z axis from
    (4, 2, -10), along the face x = 4 of the copies' box.
    The pick finds the quad's edge at (4, 2, 1), and the debug frame equals the oracle's."""
    S = ts.exact_scene(gpu_device)
    r, blob = S.frame("debug")
    o, d = oracle.camera_rays(blob, [[0.5, 0.5]])
    bh, _ = ts.brute_force(S.tri9, S.flags, np.array([[*o[0], 0.0]], np.float32),
                           np.array([[*d[0], np.inf]], np.float32))
    assert _ids(bh)[0] == 0
    hit, p = gpu_device.rtPick(S.camera, 0.5, 0.5, S.scene)
    assert hit
    assert np.array_equal(np.array(p, np.float32), o[0] + bh[0, 0] * d[0]), p
    img = S.render(r, 64)
    ref, _ = oracle.render(blob, 64, 64, 1.0)
    assert np.array_equal(img, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["chain", "exact"])
def test_guides_equal_ray_queries(gpu_device, chain_gpu, which):
    """One closest-hit rule on the device: the guide pass (k_guides, closest_hit with its private
    stack) and the ray-query kernel (yrtIntersect, k_trace) answer the same 64 x 64 pixel-centre
    camera rays alike: the guides' hit mask (pos4.w < inf) is the query's tri >= 0, and pos4.w
    is the query's t bit for bit on every hit; both equal brute force. The rays are the oracle's
    camera rays through ((x + .5) / 64, (y + .5) / 64), the kernel's own (exact quotients). On the
    chain every one of them reaches stack height >= 34 (test_chain_camera_rays_are_deep), where
    k_trace spills."""
    S = chain_gpu if which == "chain" else ts.exact_scene(gpu_device)
    pos, _ = gpu_device.render_guides(S.camera, S.scene, 64, 64)
    gt = np.ascontiguousarray(pos[..., 3], np.float32).reshape(-1)
    px = (np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).reshape(-1, 2) + 0.5) / 64.0
    o, d = oracle.camera_rays(S.blob, px)
    org = np.concatenate([o, np.zeros((len(o), 1), np.float32)], 1)
    dr = np.concatenate([d, np.full((len(d), 1), np.inf, np.float32)], 1)
    h, _ = _query(gpu_device, S.scene, org, dr)
    bh, _ = ts.brute_force(S.tri9, S.flags, org, dr)
    hit = gt < np.inf
    print(which, "guide hits:", int(hit.sum()), "of", len(gt))
    assert 0 < hit.sum()
    for name, ref in (("yrtIntersect", h), ("brute force", bh)):
        assert np.array_equal(hit, _ids(ref) >= 0), (name, np.flatnonzero(hit != (_ids(ref) >= 0))[:8])
        bad = np.flatnonzero(_bits(gt[hit]) != _bits(ref[hit, 0]))
        assert len(bad) == 0, (name, len(bad), gt[hit][bad[:4]], ref[hit, 0][bad[:4]])
