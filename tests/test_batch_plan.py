"""The wavefront job's batch plan (csrc/device/render_job.cpp plan_batches), through the device
library's host-side export yrtDebugBatchPlan (CPU only). The plan decides speed alone: every plan
renders the same pixels, so the invariance tests (test_batch_capacity_invariance,
test_lanes_invariance, tests/test_cubes.py) pass whatever it is. Here the C function is held to
the formula, restated in Python below, and to a table of the jobs the measurements were made on
(profiles/r04/ab_r04k.txt)."""
import ctypes as C

import pytest

from yrt import _native as N

Mi = 1 << 20
DEFAULT_CAPACITY = 64 * Mi


def plan_py(shard_tiles, spp, capacity, lanes, capture, grow):
    """(tilesPerBatch, numBatches, pathsPerBatch, lanes used)"""
    tiles_per_batch = max(1, capacity // (256 * spp))
    if not capture and lanes > 1 and shard_tiles > 1:
        nb = (shard_tiles + tiles_per_batch - 1) // tiles_per_batch
        nb = (nb + lanes - 1) // lanes * lanes
        g = grow and capacity == DEFAULT_CAPACITY
        if g and 4 * lanes < nb <= 8 * lanes:
            nb = (nb // 2 + lanes - 1) // lanes * lanes
        elif g and 8 * lanes < nb <= 16 * lanes:
            nb = (nb * 2 // 3 + lanes - 1) // lanes * lanes
        tiles_per_batch = (shard_tiles + nb - 1) // nb
    paths = min(tiles_per_batch, shard_tiles) * 256 * spp
    num_batches = (shard_tiles + tiles_per_batch - 1) // tiles_per_batch
    used = 1 if capture else max(1, min(lanes, num_batches))
    return tiles_per_batch, num_batches, paths, used


def plan_c(shard_tiles, spp, capacity, lanes, capture, grow):
    out = (C.c_int64 * 4)()
    assert N.dev.yrtDebugBatchPlan(shard_tiles, spp, capacity, lanes, capture, grow, out) == 0
    return tuple(out)


# (shardTiles, spp, capacity, lanes, capture, grow) -> (tilesPerBatch, numBatches, pathsPerBatch, lanes used)
TABLE = [
    ((16384, 64, 64 * Mi, 3, 0, 1), (2731, 6, 44744704, 3)),       # C3
    ((110592, 256, 64 * Mi, 3, 0, 1), (1024, 108, 67108864, 3)),   # C4 cube job
    ((110592, 256, 64 * Mi, 4, 0, 1), (1024, 108, 67108864, 4)),   # four lanes
    ((13824, 256, 64 * Mi, 3, 0, 1), (1536, 9, 100663296, 3)),     # C4 N = 8 share: halving band (15 -> 9)
    ((13824, 256, 64 * Mi, 3, 0, 0), (922, 15, 60424192, 3)),      # same, grow off
    ((27648, 256, 64 * Mi, 3, 0, 1), (1536, 18, 100663296, 3)),    # x2/3 band (27 -> 18)
    ((55296, 256, 64 * Mi, 3, 0, 1), (1024, 54, 67108864, 3)),     # above both bands
    ((16384, 64, 16 * Mi, 3, 0, 1), (911, 18, 14925824, 3)),       # non-default capacity never grows
    ((16384, 64, 64 * Mi, 1, 0, 1), (4096, 4, 67108864, 1)),       # one lane: no rounding
    ((16384, 64, 64 * Mi, 3, 4096, 1), (4096, 4, 67108864, 1)),    # capture frame: one lane
    ((1, 64, 64 * Mi, 3, 0, 1), (4096, 1, 16384, 1)),              # one tile
    ((2, 64, 64 * Mi, 3, 0, 1), (1, 2, 16384, 2)),                 # fewer batches than lanes
    ((16, 4, 64 * Mi, 3, 0, 1), (6, 3, 6144, 3)),                  # the tests' own small frames
]


@pytest.mark.parametrize("args,want", TABLE)
def test_plan_table(args, want):
    assert plan_py(*args) == want
    assert plan_c(*args) == want


def test_c_plan_follows_the_formula():
    """Every band edge of the grow rule for 1-4 lanes, at and beside the default capacity."""
    for lanes in (1, 2, 3, 4):
        for spp in (1, 4, 64, 256):
            per = DEFAULT_CAPACITY // (256 * spp)
            tiles = {1, 2, 3, lanes, lanes + 1, per - 1, per, per + 1}
            for nb in (4, 8, 16):  # the bands' edges in batches per lane
                for d in (-1, 0, 1):
                    tiles.add(max(1, (nb * lanes + d) * per))
                    tiles.add(max(1, (nb * lanes + d) * per + 1))
            for capacity in (DEFAULT_CAPACITY, DEFAULT_CAPACITY // 4, DEFAULT_CAPACITY + 256, 256):
                for t in sorted(tiles):
                    for capture in (0, 1):
                        for grow in (0, 1):
                            a = (t, spp, capacity, lanes, capture, grow)
                            assert plan_c(*a) == plan_py(*a), a


def test_plan_covers_the_shard():
    for t in (1, 2, 7, 16, 1000, 13824, 110592):
        for lanes in (1, 2, 3, 4):
            tpb, nb, paths, used = plan_c(t, 256, DEFAULT_CAPACITY, lanes, 0, 1)
            assert (nb - 1) * tpb < t <= nb * tpb and 1 <= used <= min(lanes, nb)
            assert paths == min(tpb, t) * 256 * 256


def test_invalid_arguments():
    out = (C.c_int64 * 4)()
    for a in [(-1, 64, 64 * Mi, 3, 0, 1), (16, 0, 64 * Mi, 3, 0, 1), (16, 64, 0, 3, 0, 1), (16, 64, 64 * Mi, 0, 0, 1)]:
        assert N.dev.yrtDebugBatchPlan(*a, out) == -1
    assert N.dev.yrtDebugBatchPlan(16, 64, 64 * Mi, 3, 0, 1, None) == -1
