"""A numpy model of the multi-GPU gather's tile slab, written from the documented layout
(csrc/kernels/yrt_kernels.h, "Multi-GPU gather"; csrc/common/yrt_tile_scatter.h), not from the
kernels. It uses no project library: tests/test_tile_slab.py compares k_pack_tiles and
k_unpack_tiles with it bit for bit.

The layout. A job is `frames` images of W x H pixels stacked in memory, cut into 16 x 16 tiles in
scan order, ntx = ceil(W / 16) tiles per row and nty = ceil(H / 16) rows, tilesPerFrame = ntx * nty;
job tile t lies in frame t // tilesPerFrame. A shard (offset, stride) owns the job tiles
offset + j * stride; its slab holds them in the order of j, 256 elements per tile in scan order
within the tile (element 16 * row + column). When the job is sharded (stride > 1) the tile's index
within its frame is a logical one: it covers image tile tile_scatter(index, tilesPerFrame). A
slab element is one 32-bit word r | g << 8 | b << 16 of the RGB8 bytes (rgb8), or four 32-bit
words: the float pixel's r, g, b and that same RGB8 word. Elements of a tile that overhang the
image are zero in a packed slab and are skipped on unpack. RGB8 frames are byte rows of
rgb8_row_stride(W) bytes, three per pixel and up to three of padding.

Float pixels are handled as uint32 words throughout, so NaN payloads and signed zeros survive.
"""
from functools import lru_cache

import numpy as np

TILE = 16


def rgb8_row_stride(W):
    """Bytes per row of an RGB8 frame: 3 * W rounded up to a multiple of 4."""
    return (3 * W + 3) // 4 * 4


def tiles_per_frame(W, H):
    return ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)


def shard_tiles(num_tiles, offset, stride):
    """How many of the job's num_tiles tiles the shard offset + j * stride owns."""
    return (num_tiles - offset + stride - 1) // stride if num_tiles > offset else 0


def _mix(x, m, h):
    x = (x * 0x9E3779B1) & m
    x ^= x >> h
    x = (x * 0x85EBCA6B) & m
    x ^= x >> h
    return x


def tile_scatter(t, T):
    """The image tile that logical tile t of a sharded job's frame of T tiles covers: a bijection
    of [0, 2^B), 2^B >= T (two rounds of an odd multiply mod 2^B and a right xorshift by
    ceil(B / 2)), walked along its cycle until the value is below T. The identity for T <= 2."""
    if not 0 <= t < T:
        raise ValueError((t, T))
    if T <= 2:
        return t
    B = (T - 1).bit_length()
    m, h = (1 << B) - 1, (B + 1) >> 1
    x = _mix(t, m, h)
    while x >= T:
        x = _mix(x, m, h)
    return x


@lru_cache(maxsize=32)
def scatter_table(T):
    """tile_scatter(t, T) for every t, int64 (T,) (vectorised: the products stay below 2^63)."""
    x = np.arange(T, dtype=np.uint64)
    if T > 2:
        B = (T - 1).bit_length()
        m, h = np.uint64((1 << B) - 1), np.uint64((B + 1) >> 1)
        todo = np.ones(T, bool)
        while todo.any():
            x[todo] = _mix(x[todo], m, h)
            todo &= x >= np.uint64(T)
    out = x.astype(np.int64)
    out.setflags(write=False)
    return out


def slab_index(W, H, frames, offset, stride, num_tiles):
    """(f, x, y, inside) of every element of the shard's slab, int64 / bool (num_tiles * 256,):
    the frame, the pixel, and whether the pixel lies inside the image."""
    ntx = (W + TILE - 1) // TILE
    tpf = tiles_per_frame(W, H)
    if offset < 0 or stride < 1 or num_tiles < 0 or num_tiles > shard_tiles(tpf * frames, offset, stride):
        raise ValueError("the shard does not hold that many tiles")
    tile = offset + np.arange(num_tiles, dtype=np.int64) * stride
    f, t = tile // tpf, tile % tpf
    if stride > 1:
        t = scatter_table(tpf)[t]
    e = np.arange(256, dtype=np.int64)
    x = ((t % ntx) * TILE)[:, None] + (e % TILE)[None, :]
    y = ((t // ntx) * TILE)[:, None] + (e // TILE)[None, :]
    f = np.broadcast_to(f[:, None], x.shape)
    x, y, f = x.reshape(-1), y.reshape(-1), f.reshape(-1)
    return f, x, y, (x < W) & (y < H)


def support(W, H, frames, offset, stride, num_tiles=None):
    """bool (frames, H, W): the pixels of the shard's tiles."""
    if num_tiles is None:
        num_tiles = shard_tiles(tiles_per_frame(W, H) * frames, offset, stride)
    f, x, y, inside = slab_index(W, H, frames, offset, stride, num_tiles)
    m = np.zeros((frames, H, W), bool)
    m[f[inside], y[inside], x[inside]] = True
    return m


def _words(a, shape):
    a = np.asarray(a)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    if a.dtype != np.uint32 or a.shape != shape:
        raise ValueError((a.dtype, a.shape, shape))
    return a


def _rows(a, W, H, frames):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.shape != (frames, H, rgb8_row_stride(W)):
        raise ValueError((a.dtype, a.shape))
    return a


def pack(fb_float, fb_rgb8_rows, W, H, frames, rgb8, offset, stride, num_tiles):
    """The shard's slab of frames fb_float (float32 or uint32 (frames, H, W, 3)) and fb_rgb8_rows
    (uint8 (frames, H, rgb8_row_stride(W))): uint32 (num_tiles * 256,) with rgb8, else
    (num_tiles * 256, 4), whose float32 view is the float4 slab."""
    fw = _words(fb_float, (frames, H, W, 3))
    rows = _rows(fb_rgb8_rows, W, H, frames)
    f, x, y, inside = slab_index(W, H, frames, offset, stride, num_tiles)
    f, x, y = f[inside], x[inside], y[inside]
    c = np.zeros(num_tiles * 256, np.uint32)
    px = rows[f[:, None], y[:, None], 3 * x[:, None] + np.arange(3)[None, :]].astype(np.uint32)
    c[inside] = px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)
    if rgb8:
        return c
    slab = np.zeros((num_tiles * 256, 4), np.uint32)
    slab[inside, :3] = fw[f, y, x]
    slab[:, 3] = c
    return slab


def unpack(slab, fb_float, fb_rgb8_rows, W, H, frames, rgb8, offset, stride, num_tiles):
    """Scatters the slab into the frames, in place: the RGB8 bytes always, the float pixel too
    when the slab is float4. Overhang elements, other tiles and the rows' padding are left alone."""
    fw = _words(fb_float, (frames, H, W, 3))
    rows = _rows(fb_rgb8_rows, W, H, frames)
    s = _words(slab, (num_tiles * 256,) if rgb8 else (num_tiles * 256, 4))
    f, x, y, inside = slab_index(W, H, frames, offset, stride, num_tiles)
    f, x, y, s = f[inside], x[inside], y[inside], s[inside]
    if rgb8:
        c = s
    else:
        fw[f, y, x] = s[:, :3]
        c = s[:, 3]
    for k in range(3):
        rows[f, y, 3 * x + k] = ((c >> (8 * k)) & 0xFF).astype(np.uint8)
