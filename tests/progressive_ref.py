"""The oracle side of the progressive-frame tests (tests/test_progressive.py on the device,
tests/test_progressive_oracle.py on the CPU): what rtRenderFrame(..., accumulate=1) shows after
every call, restated with oracle.render(..., iteration=k, accu=...), and the float64 bound that
checks the accumulation itself against plain arithmetic.

Reference: IntegratorRenderer::renderFrame (renderers/integratorrenderer.cpp:63-69: accumulate=0
resets the renderer's iteration, every frame raises it), SamplerFactory::init(iteration)
(samplers/sampler.cpp:85-95) and AccuBuffer::update (api/framebuffer.h:289-304).
"""
from __future__ import annotations

import hashlib

import numpy as np

import oracle

_sequences: dict = {}
_frames: dict = {}


def _key(blob, *rest):
    return (hashlib.sha1(blob).hexdigest(),) + rest


def oracle_frame(blob: bytes, width, height, gamma, iteration):
    """The frame of sampler iteration `iteration` alone (no accumulation). Shared: do not modify."""
    k = _key(blob, width, height, float(gamma), iteration)
    if k not in _frames:
        _frames[k] = oracle.render(blob, width, height, gamma, iteration=iteration)[0]
        _frames[k].setflags(write=False)
    return _frames[k]


def oracle_sequence(blob: bytes, width, height, gamma, count):
    """What a framebuffer shows after each of `count` progressive frames from a new (or
    accumulate=0-restarted) state: iterations 0..count-1 added into one accumulation buffer.
    Computed once per (frame, count) and extended on demand. Shared: do not modify."""
    k = _key(blob, width, height, float(gamma))
    accu, shown = _sequences.setdefault(k, (np.zeros((height, width, 4), np.float32), []))
    while len(shown) < count:
        img = oracle.render(blob, width, height, gamma, iteration=len(shown), accu=accu)[0]
        img.setflags(write=False)
        shown.append(img)
    return shown[:count]


U = 2.0 ** -24  # float32 unit roundoff


def mean_bound(count):
    """eps with |D - M| <= eps * M + tiny, per channel, where D is the float32 display of `count`
    accumulated frames at gamma 1 and M the float64 mean of the same frames rendered alone.

    Per pixel and channel let L_k >= 0 be frame k's float32 sample sum, s = spp, K = count.
      single frame   F_k = fl(L_k * rcp(s))             = (L_k / s) (1 + r1) (1 + d_k)
      accumulated    S   = fl(...fl(L_0 + L_1)... + L_{K-1}) = sum_k L_k (1 + t_k)
                     w   = K s, exact (an integer below 2^24)
                     D   = fl(S * rcp(w))               = (S / (K s)) (1 + r2) (1 + d)
    with |d|, |d_k| <= u = 2^-24 (one rounding), |t_k| <= g = (K-1) u / (1 - (K-1) u) (a term of a
    sum of non-negative floats passes through at most K-1 roundings; the first addition, 0 + L_0,
    is exact), and |r1|, |r2| <= 5 u: rcp is within 2 ulp of the correctly rounded quotient
    (tests/test_sse_rcp.py::test_reference_rcp_is_not_ieee), an ulp is at most 2 u relative, and
    the correctly rounded quotient is within u. Substituting L_k / s = F_k / ((1 + r1) (1 + d_k)):
      D = (1 / K) sum_k F_k q_k,   q_k = (1 + t_k) (1 + r2) (1 + d) / ((1 + r1) (1 + d_k)),
    and since every F_k >= 0,  |D - M| <= M max_k |q_k - 1|
      <= M ((1 + g) (1 + 5 u) (1 + u) / ((1 - 5 u) (1 - u)) - 1),  about (K + 11) u.
    M itself is a float64 sum of K floats and one division: relative error below (K + 1) 2^-53.
    `tiny` covers results below the normal range (flushed or denormal): each of the K + 2
    roundings is then off by at most 2^-126 instead of relatively."""
    g = (count - 1) * U / (1 - (count - 1) * U)
    eps = (1 + g) * (1 + 5 * U) * (1 + U) / ((1 - 5 * U) * (1 - U)) - 1
    return eps + (count + 1) * 2.0 ** -53, (count + 2) * 2.0 ** -126


def check_mean(shown, singles):
    """shown: the float32 display after len(singles) accumulated frames (gamma 1); singles: those
    frames rendered alone. Asserts mean_bound and returns the largest |D - M| / (eps M + tiny)."""
    K = len(singles)
    F = np.stack([np.asarray(f, np.float64) for f in singles])
    assert np.isfinite(F).all() and (F >= 0).all(), "the bound needs finite non-negative radiance"
    M = F.sum(0) / K
    eps, tiny = mean_bound(K)
    ratio = np.abs(np.asarray(shown, np.float64) - M) / (eps * M + tiny)
    worst = float(ratio.max())
    print(f"accumulated display of {K} frames against their float64 mean: worst |D - M| / bound = {worst:.3f} "
          f"(eps = {eps:.3e})")
    assert worst <= 1.0, (worst, eps)
    return worst
