"""The multi-GPU gather's tile slabs: k_pack_tiles and k_unpack_tiles (csrc/kernels/k_tiles.h),
run as they stand through yrtDebugTileSlab, against the numpy model of the documented layout
(tests/gather_ref.py), bit for bit, at partial tiles, non-square tile grids, padded RGB8 rows,
uneven deals (one tile, no tile) and above the launch's grid cap.

Pack and unpack share one index function, so a slab that is wrong symmetrically passes every
end-to-end gather; here each kernel is compared with the model on its own. The CPU tests pin the
model itself (the scatter against the header's host build, the shard supports against
yrt.dist.tile_mask, pack/unpack round trips) and show that the shapes used tell the index
mistakes these kernels invite apart.
"""
from functools import lru_cache

import numpy as np
import pytest

import gather_ref as G
import yrt
import yrt._native as N
from test_gather import _threads
from yrt.dist import tile_mask

# (W, H, frames): one tile; two tiles with overhang in x and y (scatter the identity); 5 x 3 tiles
# per frame, RGB8 stride 212 != 210, tiles crossing a frame boundary; the transposed grid
SHAPES = [(16, 16, 1), (17, 15, 1), (70, 33, 2), (33, 70, 1)]
# 19,200 tiles: above the 16,384-block grid cap of launch_*_tiles, the grid-stride loop iterates
BIG = (640, 640, 12)
# (offset, stride); (1, 40) holds at most one tile; "none" is a deal past the job's last tile
DEALS = [(0, 1), (1, 2), (2, 3), (3, 4), (5, 7), (1, 40), "none"]
SCATTER_T = [1, 2, 3, 4, 5, 7, 15, 25, 64, 100, 169, 771]

SENT_WORD = np.uint32(0xDEADBEEF)
SENT_BYTE = np.uint8(0xCD)
SENT_SLAB = np.uint32(0xA5A5A5A5)
# NaN payloads (quiet, signalling, negative), +-0, +-inf, denormals
SPECIAL = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x00000000, 0x80000000, 0x7F800000,
                    0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000], np.uint32)


def _shape_id(shape):
    return "x".join(str(v) for v in shape)


def _deal(shape, deal):
    W, H, F = shape
    total = G.tiles_per_frame(W, H) * F
    return (total, total + 1) if deal == "none" else deal


def _tiles(shape, deal):
    W, H, F = shape
    off, st = _deal(shape, deal)
    return G.shard_tiles(G.tiles_per_frame(W, H) * F, off, st)


@lru_cache(maxsize=None)
def _frames(shape):
    """Read-only frames of random bits: float words (F, H, W, 3) with the special values strewn
    in, RGB8 rows (F, H, stride) whose padding bytes are random too."""
    W, H, F = shape
    rng = np.random.default_rng(W * 1000003 + H * 1009 + F)
    fw = rng.integers(0, 1 << 32, (F, H, W, 3), dtype=np.uint32)
    at = rng.integers(0, fw.size, max(len(SPECIAL), fw.size // 8))
    fw.reshape(-1)[at] = SPECIAL[np.arange(at.size) % len(SPECIAL)]
    rows = rng.integers(0, 256, (F, H, G.rgb8_row_stride(W)), dtype=np.uint8)
    fw.setflags(write=False)
    rows.setflags(write=False)
    return fw, rows


def _random_slab(shape, deal, rgb8):
    n = _tiles(shape, deal) * 256
    rng = np.random.default_rng(n + 7 * bool(rgb8) + 1)
    return rng.integers(0, 1 << 32, (n,) if rgb8 else (n, 4), dtype=np.uint32)


def _sentinel_frames(shape):
    W, H, F = shape
    return (np.full((F, H, W, 3), SENT_WORD, np.uint32),
            np.full((F, H, G.rgb8_row_stride(W)), SENT_BYTE, np.uint8))


# ----------------------------------------------------------------------------- the model (CPU)
@pytest.mark.parametrize("T", SCATTER_T)
def test_model_scatter_equals_the_header(T):
    got = [G.tile_scatter(t, T) for t in range(T)]
    assert got == [N.dev.yrtDebugTileScatter(t, T) for t in range(T)]
    assert sorted(got) == list(range(T))
    assert np.array_equal(G.scatter_table(T), got)
    if T == 15:
        assert got == [0, 9, 7, 1, 6, 5, 14, 2, 13, 11, 10, 3, 4, 8, 12]
    if T <= 2:
        assert got == list(range(T))


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=_shape_id)
def test_model_supports_equal_tile_mask(shape):
    """The pixels of shard (rank, world) in the model are yrt.dist.tile_mask's. A job's tiles are
    dealt frame-major, so in frame f the rank owns the logical tiles t with
    (f * tilesPerFrame + t) % world == rank: tile_mask of rank (rank - f * tilesPerFrame) % world.
    The supports of a deal's ranks partition the job."""
    W, H, F = shape
    tpf = G.tiles_per_frame(W, H)
    for world in (1, 2, 3, 4, 7, 40):
        if shape == BIG and world not in (1, 7):
            continue
        count = np.zeros((F, H, W), np.int32)
        for rank in range(world):
            m = G.support(W, H, F, rank, world)
            count += m
            for f in range(F):
                assert np.array_equal(m[f], tile_mask(W, H, (rank - f * tpf) % world, world)), (world, rank, f)
        assert (count == 1).all(), world


@pytest.mark.parametrize("rgb8", [0, 1], ids=["float4", "rgb8"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_model_pack_unpack_reproduces_the_shard(shape, rgb8):
    """pack, then unpack into zeroed frames: exactly the shard's pixels, nothing else."""
    W, H, F = shape
    fw, rows = _frames(shape)
    for deal in DEALS:
        off, st = _deal(shape, deal)
        n = _tiles(shape, deal)
        slab = G.pack(fw, rows, W, H, F, rgb8, off, st, n)
        f, x, y, inside = G.slab_index(W, H, F, off, st, n)
        assert not slab[~inside].any()
        out_w, out_r = np.zeros_like(fw), np.zeros_like(rows)
        G.unpack(slab, out_w, out_r, W, H, F, rgb8, off, st, n)
        m = G.support(W, H, F, off, st)
        assert m.sum() == inside.sum()
        want_r = np.zeros_like(rows)
        want_r[:, :, :3 * W] = (rows[:, :, :3 * W].reshape(F, H, W, 3) * m[..., None]).reshape(F, H, 3 * W)
        assert np.array_equal(out_r, want_r), deal
        assert np.array_equal(out_w, np.zeros_like(fw) if rgb8 else fw * m[..., None]), deal


def _variant_index(W, H, F, off, st, n, swap_grid=False, no_scatter=False, swap_xy=False):
    """gather_ref.slab_index restated with one of the mistakes the kernels' index function
    invites: the row tile count where the column tile count belongs, the scatter left out, the
    in-tile x and y exchanged."""
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    per_row = nty if swap_grid else ntx
    tile = off + np.arange(n, dtype=np.int64) * st
    f, t = tile // (ntx * nty), tile % (ntx * nty)
    if st > 1 and not no_scatter:
        t = G.scatter_table(ntx * nty)[t]
    e = np.arange(256, dtype=np.int64)
    ex, ey = (e // 16, e % 16) if swap_xy else (e % 16, e // 16)
    x = ((t % per_row) * 16)[:, None] + ex[None, :]
    y = ((t // per_row) * 16)[:, None] + ey[None, :]
    f = np.broadcast_to(f[:, None], x.shape).reshape(-1)
    x, y = x.reshape(-1), y.reshape(-1)
    return f, x, y, (x < W) & (y < H)


def _cases_that_separate(variant):
    """The (shape, deal) cases at which a variant's slab differs from the model's: some element is
    inside the image for one of the two and is not the same pixel for both (the frames' pixels
    are random, so another pixel is another value)."""
    out = []
    for shape in SHAPES:
        W, H, F = shape
        for deal in DEALS:
            off, st = _deal(shape, deal)
            n = _tiles(shape, deal)
            a = G.slab_index(W, H, F, off, st, n)
            if variant == "rgb8Stride = 3W":
                # rows read at a stride of 3W bytes instead of rgb8_row_stride(W)
                fw, rows = _frames(shape)
                tight = np.zeros_like(rows)
                tight[:, :, :3 * W] = rows.reshape(-1)[:F * H * 3 * W].reshape(F, H, 3 * W)
                differs = not np.array_equal(G.pack(fw, rows, W, H, F, 1, off, st, n),
                                             G.pack(fw, tight, W, H, F, 1, off, st, n))
            else:
                b = _variant_index(W, H, F, off, st, n, **{variant: True})
                other = (a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3])
                differs = bool(((a[3] | b[3]) & other).any())
            if differs:
                out.append((shape, deal))
    return out


def test_the_shapes_tell_mutants_apart():
    """The reference only: each of four wrong variants of the model differs from it at some case
    of the list the GPU tests run, so those inputs are not blind to these mistakes. The unchanged
    restatement differs nowhere. At 96 x 96 (what the rendered gathers use) the grid variant is
    invisible."""
    for shape in SHAPES:
        for deal in DEALS:
            W, H, F = shape
            off, st = _deal(shape, deal)
            n = _tiles(shape, deal)
            a, b = G.slab_index(W, H, F, off, st, n), _variant_index(W, H, F, off, st, n)
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
    seen = {v: _cases_that_separate(v) for v in ("swap_grid", "no_scatter", "swap_xy", "rgb8Stride = 3W")}
    for v, cases in seen.items():
        assert cases, f"no case separates the variant '{v}'"
    grid = {s for s, _ in seen["swap_grid"]}
    assert (70, 33, 2) in grid and (33, 70, 1) in grid
    assert ((70, 33, 2), (0, 1)) in seen["swap_grid"]  # without the scatter's help too
    assert {s for s, _ in seen["rgb8Stride = 3W"]} == {(17, 15, 1), (70, 33, 2), (33, 70, 1)}
    a = G.slab_index(96, 96, 1, 1, 2, 18)
    b = _variant_index(96, 96, 1, 1, 2, 18, swap_grid=True)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


# ----------------------------------------------------------------------------- the probe's refusals
# (W, H, frames, offset, stride, tiles, op, slab elements or None for what the job needs) -> message
VALID = (17, 15, 1, 0, 1, 2, 0, None)
REFUSED = [
    ((0, 15, 1, 0, 1, 0, 0, None), "invalid arguments"),
    ((17, 0, 1, 0, 1, 0, 0, None), "invalid arguments"),
    ((17, 15, 0, 0, 1, 0, 0, None), "invalid arguments"),
    ((-17, 15, 1, 0, 1, 0, 0, None), "invalid arguments"),
    ((17, 15, 1, 0, 0, 1, 0, None), "invalid arguments"),
    ((17, 15, 1, 0, -1, 1, 0, None), "invalid arguments"),
    ((17, 15, 1, -1, 1, 1, 0, None), "invalid arguments"),
    ((17, 15, 1, 0, 1, -1, 0, None), "invalid arguments"),
    ((17, 15, 1, 0, 1, 2, 2, None), "invalid arguments"),
    ((17, 15, 1, 0, 1, 3, 0, None), "exceeds the shard's tiles"),
    ((17, 15, 1, 1, 2, 2, 1, None), "exceeds the shard's tiles"),
    ((17, 15, 1, 2, 1, 1, 0, None), "exceeds the shard's tiles"),
    ((17, 15, 1, 1, 2 ** 31 - 1, 2, 0, None), "exceeds the shard's tiles"),
    ((17, 15, 1, 0, 1, 2, 0, 511), "smaller than the job"),
    ((17, 15, 1, 0, 1, 2, 1, 511), "smaller than the job"),
]


def _refused(dev, args, rgb8, msg):
    """The call fails with `msg` and leaves every buffer as it was."""
    W, H, F, off, st, n, op, elems = args
    fw, rows = _sentinel_frames((max(1, abs(W)), max(1, H), max(1, F)))
    elems = max(0, n) * 256 if elems is None else elems
    slab = np.full((elems,) if rgb8 else (elems, 4), SENT_SLAB, np.uint32)
    with pytest.raises(RuntimeError, match=msg):
        dev.debug_tile_slab(op, fw, rows, slab, W, H, F, rgb8, off, st, n)
    assert (fw == SENT_WORD).all() and (rows == SENT_BYTE).all() and (slab == SENT_SLAB).all(), args


def _refusals(dev):
    for rgb8 in (0, 1):
        for args, msg in REFUSED:
            _refused(dev, args, rgb8, msg)


def test_probe_refuses_invalid_arguments(host_device):
    """Every invalid argument set is refused for its own reason, before the device is looked at;
    the valid set is refused by a host-only device. No buffer is touched."""
    _refusals(host_device)
    _refused(host_device, VALID, 0, "host-only device")
    _refused(host_device, VALID, 1, "host-only device")
    a = np.zeros((1, 15, 17, 3), np.uint32)
    with pytest.raises(ValueError):
        host_device.debug_tile_slab(0, a[:, :, ::2], np.zeros((1, 15, 52), np.uint8), np.zeros((512, 4), np.uint32),
                                    17, 15, 1, 0, 0, 1, 2)


def test_hub_moves_a_zero_byte_slab():
    """A rank that owns no tile sends a slab of zero bytes: the hub's send and receive complete."""
    hub = yrt.ShardHub(2)
    for _ in range(2):
        assert _threads([lambda: hub.status(0, 1, 5.0), lambda: hub.status(1, 1, 5.0)]) == [1, 1]
        res = _threads([lambda: hub.slab(0, recv_bytes_per_rank=0, timeout=5.0), lambda: hub.slab(1, b"", timeout=5.0)])
        assert not any(isinstance(r, Exception) for r in res), res
        assert res[0].tobytes() == b"" and res[1] is None
    hub.close()


# ----------------------------------------------------------------------------- the kernels (GPU)
@pytest.mark.gpu
def test_probe_refuses_invalid_arguments_on_the_gpu(gpu_device):
    _refusals(gpu_device)


def _check_pack(dev, shape, deal, rgb8):
    """The slab of the shard equals the model's, overhang zeros included; one tile of sentinel
    behind the shard's last element stays untouched (all of the slab, with no tile)."""
    W, H, F = shape
    off, st = _deal(shape, deal)
    n = _tiles(shape, deal)
    fw, rows = _frames(shape)
    fw_in, rows_in = fw.copy(), rows.copy()
    slab = np.full(((n + 1) * 256,) if rgb8 else ((n + 1) * 256, 4), SENT_SLAB, np.uint32)
    dev.debug_tile_slab(0, fw_in, rows_in, slab, W, H, F, rgb8, off, st, n)
    want = G.pack(fw, rows, W, H, F, rgb8, off, st, n)
    what = (shape, deal, rgb8)
    assert np.array_equal(slab[:n * 256], want), what
    assert (slab[n * 256:] == SENT_SLAB).all(), what
    assert np.array_equal(fw_in, fw) and np.array_equal(rows_in, rows), what


def _check_unpack(dev, shape, deal, rgb8):
    """A slab of random words (its overhang elements too) into sentinel frames: the model's
    frames. Outside the shard's tiles and in the rows' padding the sentinel stays; a float4 slab
    writes the float pixel and the RGB8 bytes, an RGB8 slab the bytes alone."""
    W, H, F = shape
    off, st = _deal(shape, deal)
    n = _tiles(shape, deal)
    slab = _random_slab(shape, deal, rgb8)
    slab_in = slab.copy()
    fw, rows = _sentinel_frames(shape)
    dev.debug_tile_slab(1, fw, rows, slab_in, W, H, F, rgb8, off, st, n)
    want_w, want_r = _sentinel_frames(shape)
    G.unpack(slab, want_w, want_r, W, H, F, rgb8, off, st, n)
    what = (shape, deal, rgb8)
    assert np.array_equal(fw, want_w), what
    assert np.array_equal(rows, want_r), what
    m = G.support(W, H, F, off, st)
    assert (fw[~m] == SENT_WORD).all(), what
    assert (rows[:, :, :3 * W].reshape(F, H, W, 3)[~m] == SENT_BYTE).all(), what
    assert (rows[:, :, 3 * W:] == SENT_BYTE).all(), what
    if rgb8:
        assert (fw == SENT_WORD).all(), what
    elif n:
        f, x, y, inside = G.slab_index(W, H, F, off, st, n)
        assert np.array_equal(fw[f[inside], y[inside], x[inside]], slab[inside, :3]), what
        assert np.array_equal(rows[f[inside], y[inside], 3 * x[inside] + 1], ((slab[inside, 3] >> 8) & 255)), what
    assert np.array_equal(slab_in, slab), what


@pytest.mark.gpu
@pytest.mark.parametrize("rgb8", [0, 1], ids=["float4", "rgb8"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_pack_equals_the_model(gpu_device, shape, rgb8):
    for deal in DEALS:
        _check_pack(gpu_device, shape, deal, rgb8)


@pytest.mark.gpu
@pytest.mark.parametrize("rgb8", [0, 1], ids=["float4", "rgb8"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_unpack_equals_the_model(gpu_device, shape, rgb8):
    for deal in DEALS:
        _check_unpack(gpu_device, shape, deal, rgb8)


@pytest.mark.gpu
@pytest.mark.parametrize("rgb8", [0, 1], ids=["float4", "rgb8"])
def test_pack_and_unpack_above_the_grid_cap(gpu_device, rgb8):
    """19,200 tiles in one shard: more blocks than launch_*_tiles' cap of 16,384, so every thread's
    grid-stride loop takes a second turn."""
    assert _tiles(BIG, (0, 1)) == 19200 > 16384
    _check_pack(gpu_device, BIG, (0, 1), rgb8)
    _check_unpack(gpu_device, BIG, (0, 1), rgb8)
