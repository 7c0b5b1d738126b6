"""The moving-geometry instantiations of the ray-query kernel, k_trace<false, true> and
k_trace<true, true> (kernels/k_trace.h), with chosen rays: what tests/test_trace_edges.py pins for
static scenes (the ring stack's spill, lane refill, ties, range edges), here with a time per ray,
through yrtIntersectTimed / yrtOccludedTimed. tri_at<true> rebuilds every leaf triangle from
p + time * m, so a lane that kept another ray's time, a contracted p + t * m or a tie broken
differently shows as a wrong id or a differing bit of t, u, v.

References: trace_scenes.brute_force with times (every ray against every triangle at the ray's
own time, numpy float32, no BVH and so no motion box), the oracle's trace with Ray::time set
(oracle.trace(..., time=...)), and for the sweep scene ids and distances written by hand. The CPU
tests pin the three against each other and show that the inputs can fail: every hand-written case
changes its answer over time, the chain's deep rays are spread over both sides of the instant at
which the backstop leaves the axis, and on the moving field a ray that is given its neighbour's
time gets another answer often enough. The GPU tests compare bit for bit; nothing here has a
tolerance.

Measured on the CPU (the asserted bounds are the issue's):
  moving chain: bvhDepth 37, greatest stack height 36 in either order; 1024 of the 4096 rays reach
  height >= 34 in closest-hit order (621 of them with time <= 0.25, 403 later) and 1099 in any-hit
  order (649 and 450); 256 axis rays have time exactly 0.25, 136 of them meet the backstop's edge.
  sweep scene: 31 cases at five times each (155 rays); 17 of the tree's 22 leaves have an odd
  triangle count, and each of the 17 is entered by a case's ray.
  moving field: given the previous ray's time, 43.3 % of the 65,536 base rays change their
  closest-hit answer and 5.3 % their occlusion flag (with motions in [-1, 1]^3: 34.5 % and 1.6 %,
  which is why trace_scenes.FIELD_MOTION is 8); a long run's chunk is 97 rays.
Measured on the MI355X: every comparison below bitwise equal. With `rtime = rayTime[q]` taken out
of the two refill sites, the long run differed in 548,464 closest-hit ids and 181,939 occlusion
flags of 1,572,901 (the chain: 718 and 718 of 4,096, the sweep table: 86 and 45 of 155); with
tri_at's p + t * m contracted to an fma, in t, u or v of 382,682 hits of the long run and 1,011
of the first 4,097 base rays (no id; the chain's and the sweep's products are exact either way).
"""
import numpy as np
import pytest

import oracle
import trace_scenes as ts
from trace_scenes import bits as _bits, compare as _compare, ids as _ids, query as _query

RING = 16                # YRT_LDS_STACK*: entries of the LDS ring
DEEP = 2 * RING + 2      # a second spilled generation, plus the kernel's parked leaf and pop-ahead
SPILL_DEPTH = 63         # the spill buffer's bound on bvhDepth (spill index <= bvhDepth - 1 - 16 < YRT_SPILL_1 = 48)


def _oracle(S, org, dr, time):
    """(closest hits, occlusion flags) of the oracle with Ray::time = time."""
    return oracle.trace(S.blob, org, dr, time=time), _ids(oracle.trace(S.blob, org, dr, any_hit=True, time=time))


def _references(S, org, dr, time):
    """(closest hits, occlusion flags): brute force at the rays' times, checked against the oracle
    bit for bit (t, u, v of hits, ids, flags)."""
    bh, bo = ts.brute_force(S.tri9, S.flags, org, dr, S.mot9, time)
    ref, ref_occ = _oracle(S, org, dr, time)
    bad = np.flatnonzero(_ids(bh) != _ids(ref))
    assert len(bad) == 0, (len(bad), bad[:8], _ids(bh)[bad[:8]], _ids(ref)[bad[:8]])
    m = _ids(bh) >= 0
    assert np.array_equal(_bits(bh[m, :3]), _bits(ref[m, :3]))
    assert np.array_equal(bo, ref_occ)
    return bh, bo


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _leaves(S):
    """(first slot, count) of every leaf of the device's own tree, from the quantized nodes'
    child words (slot << 5 | count, count 0: an inner node, -1: no child)."""
    q, tris, tb = S.bvh()
    child = q.reshape(-1, 64)[:, 16:32].copy().view(np.int32).reshape(-1)
    child = child[(child != -1) & ((child & 31) > 0)]
    first, count = child >> 5, child & 31
    assert count.sum() == tris.nbytes // tb  # every leaf record belongs to exactly one leaf
    return first, count


# ============================================================================= CPU
@pytest.fixture(scope="module")
def chain_cpu(host_device):
    S = ts.moving_chain_scene(host_device)
    org, dr, kind = ts.chain_rays(S.tri9)
    return (S,) + _frozen(org, dr, ts.chain_times(len(org)), kind)


@pytest.fixture(scope="module")
def sweep_cpu(host_device):
    return ts.sweep_scene(host_device)


@pytest.fixture(scope="module")
def field_cpu(host_device):
    """The moving field on the host device, its base rays and the oracle's answers to them."""
    S = ts.moving_field_scene(host_device)
    org, dr, time = ts.moving_field_base(S)
    ref, ref_occ = _oracle(S, org, dr, time)
    return (S,) + _frozen(org, dr, time, ref, ref_occ)


def test_timed_queries_need_a_gpu(host_device, sweep_cpu):
    """A host-only device refuses the timed calls as it refuses the untimed ones (before any
    pointer is looked at)."""
    S = sweep_cpu
    for time_ptr in (None, 0):
        with pytest.raises(RuntimeError, match="host-only"):
            host_device.intersect(S.scene, 0, 0, 0, 0, time_ptr=time_ptr)
        with pytest.raises(RuntimeError, match="host-only"):
            host_device.occluded(S.scene, 0, 0, 0, 0, time_ptr=time_ptr)


def test_moving_chain_brute_force_equals_oracle(chain_cpu):
    """The two references agree on the 4096 chain rays at their times, and the axis rays' answer
    follows the time alone: the backstop for time < 0.25, nothing for time > 0.25 (the ranges cut
    short miss it at any time)."""
    S, org, dr, time, kind = chain_cpu
    assert S.has_motion and b"motions" in S.blob
    assert np.array_equal(oracle.scene_triangles(S.blob), S.tri9)
    bh, bo = _references(S, org, dr, time)
    i = np.arange(len(org))
    axis = (kind < 2) & ((i // 4) % 4 != 3)
    got = _ids(bh)
    assert (got[axis & (time < 0.25)] == ts.CHAIN_WALL).all() and (got[axis & (time > 0.25)] == -1).all()
    assert (got[(kind < 2) & ~axis] == -1).all()
    at = got[axis & (time == 0.25)]
    print("axis rays at exactly 0.25:", len(at), "of them on the backstop's edge or inside:", int((at >= 0).sum()))
    assert len(at) >= 64
    # every wave of 64 holds times on both sides of 0.25 and the three exact ones
    w = time.reshape(-1, 64)
    assert ((w < 0.25).any(1) & (w > 0.25).any(1) & (w == 0).any(1) & (w == 0.25).any(1) & (w == 1).any(1)).all()
    # at time 0 the moving scene is the static chain: the same answers as without times
    sh, so = ts.brute_force(S.tri9, S.flags, org, dr)
    zh, zo = ts.brute_force(S.tri9, S.flags, org, dr, S.mot9, np.zeros(len(org), np.float32))
    assert np.array_equal(_bits(sh), _bits(zh)) and np.array_equal(so, zo)
    assert not np.array_equal(_ids(sh), got)


def test_moving_chain_reaches_the_spill(chain_cpu):
    """The deep descent of the static chain test, with times: bvhDepth between 36 and 63 (the
    spill buffer's bound); at least 64 rays in each order reach 34 stack entries, and of those at
    least a quarter have time <= 0.25 (the backstop, pushed first and popped last, is hit) and at
    least a quarter time > 0.25 (it is missed).
    oracle.traverse_stats knows no motion: it walks the exported tree with the leaf triangles as
    they are at time 0. That is sound for the stack heights here, because the chain does not move
    (every box and triangle test on the way down is the same at any time) and the backstop is
    popped last, after the greatest height has been reached."""
    S, org, dr, time, kind = chain_cpu
    depth = S.info["bvhDepth"]
    print("moving chain: bvhDepth", depth)
    assert 36 <= depth <= SPILL_DEPTH
    q, tris, tb = S.bvh()
    for any_hit in (False, True):
        h = oracle.traverse_stats(q, tris, org, dr, any_hit=any_hit, tri_bytes=tb)[0]
        deep = h >= DEEP
        early, late = int((time[deep] <= 0.25).sum()), int((time[deep] > 0.25).sum())
        print("any" if any_hit else "closest", "max height", h.max(), "rays >= 34:", int(deep.sum()),
              "with time <= 0.25:", early, "with time > 0.25:", late)
        assert h.max() <= depth
        assert deep.sum() >= 64
        assert 4 * early >= deep.sum() and 4 * late >= deep.sum()
        per_wave = h.reshape(-1, 64)
        assert ((per_wave >= DEEP).any(1) & (per_wave <= RING - 3).any(1)).all()


def test_sweep_cases_three_ways(sweep_cpu):
    """Hand-written ids and distances, brute force and the oracle agree on every case at every
    time; the occlusion flag is 'some triangle accepted'. Every case has two times with different
    expected answers: a kernel that ignored the time, or used one time for the five adjacent
    rays, would fail it."""
    S = sweep_cpu
    assert S.has_motion and np.array_equal(oracle.scene_triangles(S.blob), S.tri9)
    assert len(S.tri9) == ts.SW_COPIES + 2 * ts.SWEEP_COPIES
    # every vertex at every time, and so every product of the triangle test, is exact
    for t in ts.SWEEP_TIMES:
        p = S.tri9.astype(np.float64) + t * S.mot9.astype(np.float64)
        assert np.array_equal(p, np.round(p)) and np.abs(p).max() <= 64
    org, dr, time, want, want_t, names = ts.sweep_rays()
    print("sweep cases:", len(org) // 5, "at", len(ts.SWEEP_TIMES), "times:", len(org), "rays")
    assert len(org) % 5 == 0 and np.array_equal(time.reshape(-1, 5), np.tile(np.float32(ts.SWEEP_TIMES), (len(org) // 5, 1)))
    bh, bo = _references(S, org, dr, time)
    got = _ids(bh)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(names[i], int(want[i]), int(got[i])) for i in bad[:8]]
    m = want >= 0
    assert np.array_equal(bh[m, 0], want_t[m]), [names[i] for i in np.flatnonzero(m & (bh[:, 0] != want_t))[:8]]
    assert np.array_equal(bo, m.astype(np.int32))
    answer = np.stack([want, np.where(m, want_t, 0).view(np.int32)], 1).reshape(-1, 5, 2)
    same = [(answer[k] == answer[k, 0]).all() for k in range(len(answer))]
    assert not any(same), [names[5 * k] for k in np.flatnonzero(same)]
    # every kind of case is there
    for tri in (ts.SW_QUAD_A, ts.SW_QUAD_B, ts.SW_ALONG, ts.SW_COLLAPSE, ts.SW_FLIP, ts.SW_STATIC, ts.SW_APPROACH,
                ts.SW_APPROACH2, ts.SW_STATIC2, ts.SW_COVER_A, ts.SW_COVER_B, ts.SW_COPIES, ts.SW_COPIES + 1):
        assert (want == tri).any(), tri
    assert (want[time == 0] >= 0).any() and (want[time == 1] >= 0).any()


def test_sweep_rays_walk_leaves_with_a_remainder(sweep_cpu):
    """The device's own tree of the sweep scene has leaves whose triangle count is odd, so that
    their last leaf step takes fewer than kTriStep = 2 triangles, and some case's ray enters one:
    its (x, y) lies in the leaf's box over the whole frame time, and the box's span in z meets the
    ray between tnear and the hit the ray ends with (every box test on the way is then passed:
    the kernel tests against the closest hit so far, which is no nearer)."""
    S = sweep_cpu
    assert S.info["bvhDepth"] <= SPILL_DEPTH
    first, count = _leaves(S)
    _, tris = S.dev.export_bvh(S.scene)
    tb = S.info["triRecordBytes"]
    gid = tris.reshape(-1, tb)[:, 12:16].copy().view(np.int32)[:, 0]
    org, dr, time, want, want_t, names = ts.sweep_rays()
    end = np.where(want >= 0, want_t, dr[:, 3])
    odd = np.flatnonzero(count % 2 == 1)
    entered = 0
    for k in odd:
        g = gid[first[k]:first[k] + count[k]]
        p = np.concatenate([S.tri9[g].reshape(-1, 3), (S.tri9[g] + S.mot9[g]).reshape(-1, 3)])
        lo, hi = p.min(0), p.max(0)
        inside = ((org[:, :2] >= lo[:2]) & (org[:, :2] <= hi[:2])).all(1)
        a, b = (lo[2] - org[:, 2]) / dr[:, 2], (hi[2] - org[:, 2]) / dr[:, 2]
        near, far = np.maximum(np.minimum(a, b), org[:, 3]), np.minimum(np.maximum(a, b), end)
        entered += bool((inside & (near <= far)).any())
    print("sweep scene: leaves", len(count), "with an odd count:", len(odd), "entered by a case's ray:", entered)
    assert len(odd) >= 1 and entered >= 1


def test_moving_field_brute_force_equals_oracle(field_cpu):
    """Brute force at the rays' times equals the oracle on the first 4,096 base rays; hits and
    misses, occluded and free rays are all well represented."""
    S, org, dr, time, ref, ref_occ = field_cpu
    assert np.array_equal(oracle.scene_triangles(S.blob), S.tri9) and len(S.tri9) == 782 + 558
    assert (S.mot9[:782] != 0).any() and not S.mot9[782:].any()
    n = 4096
    bh, bo = _references(S, org[:n], dr[:n], time[:n])
    assert np.array_equal(_bits(bh[_ids(bh) >= 0]), _bits(ref[:n][_ids(bh) >= 0])) and np.array_equal(bo, ref_occ[:n])
    print("moving field: hit share", (_ids(bh) >= 0).mean(), "on the moving mesh", (_ids(bh)[_ids(bh) >= 0] < 782).mean())
    assert 0.25 < (_ids(bh) >= 0).mean() < 0.9 and 0.25 < bo.mean() < 0.9
    assert ((_ids(bh) >= 0) & (_ids(bh) < 782)).mean() > 0.25


def test_moving_field_stale_times_change_answers(field_cpu):
    """What a stale time would cost: with the times rolled by one ray (every ray given the time
    of the ray before it, as a lane that kept its previous ray's time roughly would), the oracle's
    closest hit differs on at least a quarter of the base rays and its occlusion flag on at least
    a twentieth. The long run draws its 2^20 + 2^19 + 37 rays from this base set, in chunks longer
    than a wave, so every lane is refilled in flight with a ray of another time."""
    S, org, dr, time, ref, ref_occ = field_cpu
    i = np.arange(len(org))
    assert (time[i % 16 == 0] == 0).all() and (time[i % 16 == 1] == 1).all() and 0 <= time.min() and time.max() <= 1
    stale = np.roll(time, 1)
    sref, socc = _oracle(S, org, dr, stale)
    differs = (_ids(sref) != _ids(ref)) | ((_ids(ref) >= 0) & (_bits(sref[:, 0]) != _bits(ref[:, 0])))
    share, share_occ = differs.mean(), (socc != ref_occ).mean()
    print("moving field: stale time changes the closest hit of", share, "and the occlusion flag of", share_occ)
    assert share >= 1 / 4
    assert share_occ >= 1 / 20
    chunk, waves = ts.launch_chunk(ts.LONG_N)
    print("long run: chunk", chunk, "waves", waves)
    assert chunk > 64 and (chunk, waves) == (97, 16384)
    # the void kinds of refill_base return nothing at any time, the rest still hits
    void = (i % 4 == 1) & ((i // 4) % 4 < 3)
    assert (_ids(ref)[void] == -1).all() and (_ids(ref)[i % 4 != 1] >= 0).mean() > 0.25


# ============================================================================= GPU
@pytest.fixture(scope="module")
def chain_gpu(gpu_device):
    S = ts.moving_chain_scene(gpu_device)
    assert S.info["bvhDepth"] <= SPILL_DEPTH  # before any launch: the spill index stays below YRT_SPILL_1
    return S


@pytest.fixture(scope="module")
def field_gpu(gpu_device):
    """The moving field on the GPU device, its base rays and the oracle's answers, computed once."""
    S = ts.moving_field_scene(gpu_device)
    assert S.info["bvhDepth"] <= SPILL_DEPTH
    org, dr, time = ts.moving_field_base(S)
    ref, ref_occ = _oracle(S, org, dr, time)
    return (S,) + _frozen(org, dr, time, ref, ref_occ)


@pytest.mark.gpu
def test_moving_chain_queries_gpu(gpu_device, chain_gpu):
    """Spill under MOTION: the 4096 chain rays with their times through the timed calls equal
    brute force and the oracle (ids and flags exact, t, u, v bitwise); the device's own tree is as
    deep as the host build's."""
    S = chain_gpu
    org, dr, _ = ts.chain_rays(S.tri9)
    time = ts.chain_times(len(org))
    q, tris, tb = S.bvh()
    for any_hit in (False, True):
        h = oracle.traverse_stats(q, tris, org, dr, any_hit=any_hit, tri_bytes=tb)[0]
        assert (h >= DEEP).sum() >= 64
    ref_hit, ref_occ = _references(S, org, dr, time)
    _compare(*_query(gpu_device, S.scene, org, dr, time=time), ref_hit, ref_occ)


@pytest.mark.gpu
def test_sweep_cases_gpu(gpu_device):
    """The sweep scene's hand-written table through both timed calls."""
    S = ts.sweep_scene(gpu_device)
    assert S.info["bvhDepth"] <= SPILL_DEPTH
    assert (_leaves(S)[1] % 2 == 1).any()
    org, dr, time, want, want_t, names = ts.sweep_rays()
    ref_hit, ref_occ = _references(S, org, dr, time)
    h, c = _query(gpu_device, S.scene, org, dr, time=time)
    bad = np.flatnonzero(_ids(h) != want)
    assert len(bad) == 0, [(names[i], int(want[i]), int(_ids(h)[i])) for i in bad[:8]]
    m = want >= 0
    assert np.array_equal(h[m, 0], want_t[m]) and np.array_equal(c, m.astype(np.int32))
    _compare(h, c, ref_hit, ref_occ)


@pytest.mark.gpu
def test_moving_field_long_run(gpu_device, field_gpu):
    """Lane refill under MOTION: 2^20 + 2^19 + 37 rays drawn from the base set by a fixed index
    vector give chunks of 97 rays per wave, so every lane is refilled in flight with a ray of
    another time. Every answer equals the base ray's oracle answer; every slot is written and the
    guard is not."""
    S, org, dr, time, ref, ref_occ = field_gpu
    assert ts.launch_chunk(ts.LONG_N)[0] > 64
    idx = np.random.default_rng(3).integers(0, len(org), size=ts.LONG_N)
    h, c = _query(gpu_device, S.scene, org[idx], dr[idx], time=time[idx])
    _compare(h, c, ref[idx], ref_occ[idx])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_moving_field_small_counts(gpu_device, field_gpu, n):
    S, org, dr, time, ref, ref_occ = field_gpu
    h, c = _query(gpu_device, S.scene, org, dr, n=n, time=time)
    _compare(h, c, ref[:n], ref_occ[:n])


@pytest.mark.gpu
def test_moving_field_zero_rays(gpu_device, field_gpu):
    """n = 0 with valid one-element buffers: both timed calls succeed and write nothing."""
    S, org, dr, time, _, _ = field_gpu
    h, c = _query(gpu_device, S.scene, org, dr, n=0, guard=1, time=time)
    assert len(h) == 0 and len(c) == 0


@pytest.mark.gpu
def test_time_zero_is_the_untimed_query(gpu_device, field_gpu):
    """The moving field through its camera's 64 x 64 pixel-centre rays: the timed query with every
    time 0 equals the untimed query on the same moving scene bit for bit (the untimed calls run the
    static kernels on the records as stored, which are the triangles at time 0), both equal brute
    force at time 0, and the guide pass (closest_hit, Ray's default time 0) has the same hit mask
    and the same distances in pos4.w."""
    S = field_gpu[0]
    px = (np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).reshape(-1, 2) + 0.5) / 64.0
    o, d = oracle.camera_rays(S.blob, px)
    org = np.concatenate([o, np.zeros((len(o), 1), np.float32)], 1)
    dr = np.concatenate([d, np.full((len(d), 1), np.inf, np.float32)], 1)
    zero = np.zeros(len(org), np.float32)
    th, tc = _query(gpu_device, S.scene, org, dr, time=zero)
    uh, uc = _query(gpu_device, S.scene, org, dr)
    assert np.array_equal(_bits(th), _bits(uh)) and np.array_equal(tc, uc)
    bh, bo = _references(S, org, dr, zero)
    _compare(th, tc, bh, bo)
    hit = _ids(bh) >= 0
    print("moving field: camera rays that hit:", int(hit.sum()), "of", len(hit), "on the moving mesh:",
          int((hit & (_ids(bh) < 782)).sum()))
    assert hit.sum() >= 1024 and (hit & (_ids(bh) < 782)).sum() >= 256 and (~hit).sum() >= 64
    pos, _ = gpu_device.render_guides(S.camera, S.scene, 64, 64)
    gt = np.ascontiguousarray(pos[..., 3], np.float32).reshape(-1)
    assert np.array_equal(gt < np.inf, hit), np.flatnonzero((gt < np.inf) != hit)[:8]
    bad = np.flatnonzero(_bits(gt[hit]) != _bits(th[hit, 0]))
    assert len(bad) == 0, (len(bad), gt[hit][bad[:4]], th[hit, 0][bad[:4]])


@pytest.mark.gpu
def test_static_scene_ignores_the_times(gpu_device):
    """A scene without moving geometry accepts a time array and ignores it: the timed queries on
    exact_scene with arbitrary times in [0, 1] equal the untimed ones bit for bit (the static
    kernels run; the scene has no motion records to read)."""
    S = ts.exact_scene(gpu_device)
    assert not S.has_motion and S.info["bvhDepth"] <= SPILL_DEPTH
    org, dr = ts.exact_rays()[:2]
    time = np.random.default_rng(41).uniform(0, 1, len(org)).astype(np.float32)
    time[:2] = 0.0, 1.0
    th, tc = _query(gpu_device, S.scene, org, dr, time=time)
    uh, uc = _query(gpu_device, S.scene, org, dr)
    assert np.array_equal(_bits(th), _bits(uh)) and np.array_equal(tc, uc)
    _compare(th, tc, *ts.brute_force(S.tri9, S.flags, org, dr))


@pytest.mark.gpu
def test_moving_field_on_a_morton_tree(gpu_device):
    """The moving field committed with builder "morton" (motion boxes from the GPU build), 65 and
    8,191 rays with times, tfar infinite and half of the rays cut short: equal to brute force."""
    S = ts.moving_field_scene(gpu_device)
    gpu_device.rtSetString(S.scene, "builder", "morton")
    S.commit()
    assert gpu_device.scene_build_info(S.scene)["builder"] == 1 and S.info["bvhDepth"] <= SPILL_DEPTH
    org, dr, time, far = ts.moving_field_rays(S, 8191, seed=43)
    cut = dr.copy()
    half = (np.arange(len(org)) // 3) % 2 == 0
    cut[half, 3] = far[half]
    refs = [ts.brute_force(S.tri9, S.flags, org, d, S.mot9, time) for d in (dr, cut)]
    assert (_ids(refs[0][0]) >= 0).mean() > 0.25
    assert (_ids(refs[1][0]) != _ids(refs[0][0])).mean() > 0.05  # the cut takes hits away
    for d, (ref_hit, ref_occ) in zip((dr, cut), refs):
        for n in (65, 8191):
            h, c = _query(gpu_device, S.scene, org, d, n=n, time=time)
            _compare(h, c, ref_hit[:n], ref_occ[:n])


def _sphere_motion(dev, capacity=0):
    """(frame, raysClosest) of sphere_motion at 80 x 60, 8 spp, RGB_FLOAT32 under a batch capacity."""
    import yrt
    from test_motion import MOTION
    if capacity:
        dev.set_batch_capacity(capacity)
    try:
        s = yrt.Session(MOTION + ["-size", "80", "60", "-spp", "8", "-fb", "RGB_FLOAT32"], device=dev)
        img = s.render().copy()
        rays = dev.render_stats()["raysClosest"]
        blob, gamma = s.export_frame(), s.info()["gamma"]
        s.close()
    finally:
        if capacity:
            dev.set_batch_capacity(64 << 20)
    return img, rays, blob, gamma


@pytest.mark.gpu
def test_motion_frames_across_batches_and_lanes(gpu_device, monkeypatch):
    """The per-ray times' hand-over between the queues (qTime[cur ^ 1], sTime) across batches and
    lanes: sphere_motion at 80 x 60, 8 spp in one batch, in batches of three tiles, and in those
    batches on one and on three lanes, is the same frame with the same ray count, the oracle's."""
    import yrt
    small = 256 * 8 * 3
    img, rays, blob, gamma = _sphere_motion(gpu_device)
    ref, st = oracle.render(blob, 80, 60, gamma)
    assert img.tobytes() == ref.tobytes(), np.argwhere(img != ref)[:5]
    assert rays == st["raysClosest"]
    out = [_sphere_motion(gpu_device, small)[:2]]
    for lanes in ("1", "3"):
        monkeypatch.setenv("YRT_LANES", lanes)
        d = yrt.Device(0)
        try:
            out.append(_sphere_motion(d, small)[:2])
        finally:
            d.close()
    for k, (o, r) in enumerate(out):
        assert o.tobytes() == img.tobytes(), (k, np.argwhere(o != img)[:5])
        assert r == rays, (k, r, rays)


@pytest.mark.gpu
def test_moving_field_shadow_fuse(monkeypatch):
    """The fused k_trace<true, true>: the moving field under one point light (one direct light, so
    the shadow resolve is fused into the any-hit trace) at 64 x 64, 4 spp, depth 3, with and
    without YRT_NO_SHADOW_FUSE on a fresh device each: the same frame and ray counts, the
    oracle's."""
    import yrt
    out = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("YRT_NO_SHADOW_FUSE", "1")
        else:
            monkeypatch.delenv("YRT_NO_SHADOW_FUSE", raising=False)
        d = yrt.Device(0)
        try:
            S = ts.moving_field_scene(d, light=None)
            pl = d.rtNewLight("pointlight")
            d.rtSetFloat3(pl, "P", 20.0, 12.0, 8.0)
            d.rtSetFloat3(pl, "I", 400.0, 380.0, 300.0)
            d.rtCommit(pl)
            d.rtSetPrimitive(S.scene, len(S.meshes), d.rtNewLightPrimitive(pl))
            S.commit()
            assert S.info["bvhDepth"] <= SPILL_DEPTH
            r, blob = S.frame("pathtracer", spp=4, depth=3)
            img = S.render(r, 64)
            st = d.render_stats()
            out.append((img, (st["raysClosest"], st["raysShadow"])))
        finally:
            d.close()
    ref, ost = oracle.render(blob, 64, 64, 1.0)
    print("shadow fuse:", (out[0][0] != ref).sum(), (out[1][0] != ref).sum(), "channels differ; rays", out[0][1], out[1][1],
          "lit share", (ref > 0).any(axis=2).mean())
    assert (ref > 0).any(axis=2).mean() > 0.25 and out[0][1][1] >= 1024
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1]
    assert out[0][0].tobytes() == ref.tobytes(), np.argwhere(out[0][0] != ref)[:5]
    assert out[0][1] == (ost["raysClosest"], ost["raysShadow"])
