"""The Python side of the adaptive-sampling tests (tests/test_adaptive_host.py on the CPU,
tests/test_adaptive.py on the device): the oracle's sums and half sums after n progressive
iterations, a numpy float32 restatement of the tile error estimate's exact operation sequence
(csrc/common/yrt_tile_error.h), and the same estimate in float64 arithmetic with its derived bound.

An adaptive render (yrtRenderAdaptive) adds iteration k = 0, 1, ... of the frame into the
framebuffer's sums and the even iterations into the half buffer; the oracle gives iteration k's
(L, spp) exactly: oracle.render(blob, ..., iteration=k, accu=zeros).
"""
from __future__ import annotations

import hashlib

import numpy as np

import oracle

_singles: dict = {}
_sums: dict = {}


def _key(blob, *rest):
    return (hashlib.sha1(blob).hexdigest(),) + rest


def iteration_sums(blob: bytes, width, height, k):
    """(L, spp) per pixel of sampler iteration k alone, float32 (H, W, 4). Shared: do not modify."""
    key = _key(blob, width, height, k)
    if key not in _singles:
        a = np.zeros((height, width, 4), np.float32)
        oracle.render(blob, width, height, 1.0, iteration=k, accu=a)
        a.setflags(write=False)
        _singles[key] = a
    return _singles[key]


def sums_after(blob: bytes, width, height, n):
    """(accu, half) after iterations 0..n-1: the float32 sums in the order the device adds them,
    half over the even iterations only (zeros + ...). Shared: do not modify."""
    key = _key(blob, width, height)
    seq = _sums.setdefault(key, [])
    while len(seq) < n:
        k = len(seq)
        L = iteration_sums(blob, width, height, k)
        accu = L.copy() if k == 0 else seq[-1][0] + L
        if k % 2 == 1:
            half = seq[-1][1]
        else:
            half = (np.zeros_like(L) if k == 0 else seq[-1][1]) + L
        accu.setflags(write=False)
        half.setflags(write=False)
        seq.append((accu, half))
    return seq[n - 1]


def _rcp(x):
    x = np.asarray(x, np.float32)
    return oracle.vecmath("rcp", x.reshape(-1)).reshape(x.shape)


def _rsqrt(x):
    x = np.asarray(x, np.float32)
    return oracle.vecmath("rsqrt", x.reshape(-1)).reshape(x.shape)


def _tiles(a, fill):
    """(H, W) -> (tiles_y, tiles_x, 256): each tile's pixels in scan order, outside pixels `fill`."""
    h, w = a.shape
    ty, tx = (h + 15) // 16, (w + 15) // 16
    p = np.full((ty * 16, tx * 16), fill, a.dtype)
    p[:h, :w] = a
    return p.reshape(ty, 16, tx, 16).transpose(0, 2, 1, 3).reshape(ty, tx, 256)


def _inside(width, height):
    """(tiles_y, tiles_x): the tile's pixels inside the image."""
    return _tiles(np.ones((height, width), np.int64), 0).sum(-1)


def pixel_error(accu, half):
    """e per pixel, float32 (H, W): yrt_pixel_error's operations one by one, each rounded to float32."""
    S, Hf = np.asarray(accu, np.float32), np.asarray(half, np.float32)
    with np.errstate(all="ignore"):
        rw, rh = _rcp(S[..., 3]), _rcp(Hf[..., 3])
        I = [S[..., c] * rw for c in range(3)]
        A = [Hf[..., c] * rh for c in range(3)]
        d = (np.abs(I[0] - A[0]) + np.abs(I[1] - A[1])) + np.abs(I[2] - A[2])
        s = (I[0] + I[1]) + I[2]
        e = np.where(s > 0, d * _rsqrt(s), np.float32(0))
    assert e.dtype == np.float32
    return e


def tile_error(accu, half):
    """E_T per tile, float32 (tiles_y, tiles_x): the slots in scan order, pixels outside the image 0,
    the fixed pairwise tree built by reshapes (slot i += slot i + h, h = 128 .. 1), times rcp(n_T)."""
    h, w = np.asarray(accu).shape[:2]
    v = _tiles(pixel_error(accu, half), np.float32(0))
    with np.errstate(all="ignore"):
        while v.shape[-1] > 1:
            half_len = v.shape[-1] // 2
            v = v[..., :half_len] + v[..., half_len:]
        E = v[..., 0] * _rcp(_inside(w, h).astype(np.float32))
    assert E.dtype == np.float32
    return E


U = 2.0 ** -24  # float32 unit roundoff


def tile_error_f64(accu, half):
    """(E, bound) per tile in float64 arithmetic from the same float32 sums, with true division and
    square root, and the bound |E_float32 - E| <= bound derived in
    tests/test_adaptive_host.py::test_estimate_against_float64. Needs finite non-negative sums."""
    S, Hf = np.asarray(accu, np.float64), np.asarray(half, np.float64)
    assert np.isfinite(S).all() and np.isfinite(Hf).all() and (S >= 0).all() and (Hf >= 0).all()
    h, w = S.shape[:2]
    I = S[..., :3] / S[..., 3:4]
    A = Hf[..., :3] / Hf[..., 3:4]
    d = np.abs(I - A).sum(-1)
    s, sA = I.sum(-1), A.sum(-1)
    pos = s > 0
    root = np.sqrt(np.where(pos, s, 1.0))
    e = np.where(pos, d / root, 0.0)
    a = (1 + 5 * U) * (1 + U) - 1            # a quotient S_c * rcp(w): rcp within 5 u, one product
    a1 = a * (1 + U) ** 3                     # ... carried through the subtraction and two additions
    b = (1 + a) * (1 + U) ** 2 - 1            # s: three such quotients, two additions, all >= 0
    q = 8 * U                                 # rsqrt: 3.4 u of the Newton step + 4 u of its roundings
    c = (1 + q) * (1 + U) / np.sqrt(1 - b) - 1  # d * rsqrt(s) relative to d / sqrt(s_exact)
    tiny = 16 * 2.0 ** -126                   # results below the normal range
    Bp = np.where(pos, (1 + c) * a1 * (s + sA) / root + (c + 3 * U * (1 + c)) * e, 0.0) + tiny
    n = _inside(w, h)
    t = (1 + U) ** 8 * (1 + 5 * U) * (1 + U) - 1  # eight tree levels, rcp(n_T), one product
    E = _tiles(e, 0.0).sum(-1) / n
    bound = (1 + t) * _tiles(Bp, 0.0).sum(-1) / n + t * E
    return E, bound
