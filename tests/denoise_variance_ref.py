"""numpy restatements for the variance-guided denoiser ("variance-guided"): the
per-pixel variance of a displayed frame from an adaptive render's sums and half sums, float32
operation by operation and in float64, and the float64 variance-guided a-trous filter for a single
frame, a demodulated frame and the six faces of a cube eye (tests/denoise_cube_ref.py's tap rule).
Written from the definitions, not from the kernels.

With the sums S (weight w), the half sums H (weight h) and r = w - h:
  A = H rcp(h),  B = max(S - H, 0) rcp(r),  dA = T(A), dB = T(B)   (T: pow 1 / gamma iff gamma != 1,
  f = (h r) (rcp(w) rcp(w)),  v_c = ((dA_c - dB_c)(dA_c - dB_c)) f    then the vignette iff set)
and a v_c that is not finite is 0.
"""
from __future__ import annotations

import numpy as np

import denoise_cube_ref as cref
import denoise_ref as ref
from denoise_ref import H5

F = np.float32
U = 2.0 ** -24  # float32 unit roundoff
FLOOR = float(F(1 / 255) * F(1 / 255))  # the library's varianceFloor: (1/255)^2 in float32
G3 = np.array([0.25, 0.5, 0.25])


# ----------------------------------------------------------------------------- the estimator
def _rcp(x):
    import oracle
    x = np.asarray(x, F)
    return oracle.vecmath("rcp", x.reshape(-1)).reshape(x.shape)


def frame_variance_f32(accu, half):
    """var4 (H, W, 4) float32 for gamma 1 without the vignette: every operation of the definition
    rounded to float32 in its order, rcp the reference's (oracle.vecmath)."""
    S, Hf = np.asarray(accu, F), np.asarray(half, F)
    with np.errstate(all="ignore"):
        h = Hf[..., 3]
        r = S[..., 3] - h
        rh, rr, rw = _rcp(h), _rcp(r), _rcp(S[..., 3])
        f = (h * r) * (rw * rw)
        out = np.ones(S.shape, F)
        for c in range(3):
            A = Hf[..., c] * rh
            B = np.fmax(S[..., c] - Hf[..., c], F(0)) * rr
            d = A - B
            v = (d * d) * f
            out[..., c] = np.where(np.isfinite(v), v, F(0))
    assert out.dtype == F
    return out


def display_halves_f64(accu, half, gamma=1.0, vignetting=False):
    """(dA, dB, f): the two halves as displayed, (H, W, 3) float64 each, and the factor (H, W), from
    the float32 sums in float64 arithmetic with true divisions; gamma is the tone mapper's float."""
    S, Hf = np.asarray(accu, np.float64), np.asarray(half, np.float64)
    with np.errstate(all="ignore"):
        h = Hf[..., 3]
        w = S[..., 3]
        r = w - h
        A = Hf[..., :3] / h[..., None]
        B = np.maximum(S[..., :3] - Hf[..., :3], 0.0) / r[..., None]
        if gamma != 1.0:
            e = float(_rcp(F([gamma]))[0])  # the render's own exponent: the reference's rcp of its float gamma
            A, B = A ** e, B ** e
        if vignetting:
            vig = ref.vignette(S.shape[1], S.shape[0])[..., None]
            A, B = A * vig, B * vig
        f = h * r / (w * w)
    return A, B, f


def frame_variance_f64(accu, half, gamma=1.0, vignetting=False):
    """var4 (H, W, 4) float64 by the definition."""
    A, B, f = display_halves_f64(accu, half, gamma, vignetting)
    with np.errstate(all="ignore"):
        v = (A - B) ** 2 * f[..., None]
    v = np.where(np.isfinite(v), v, 0.0)
    return np.concatenate([v, np.ones(v.shape[:2] + (1,))], -1)


# Relative error of a displayed half in float32 against display_halves_f64. The quotient H rcp(h):
# rcp within 5 u and one product, 6 u (tests/test_adaptive_host.py). gamma != 1: powf's own 2e-5
# (tests/test_libm.py); the exponent is the render's own float (display_halves_f64), so it adds
# nothing. The vignette: 2.19e-5 (tests/test_denoise.py, test_vignetting, which derives it for exactly
# this factor and product).
def display_error(gamma, vignetting):
    e = 6 * U
    if gamma != 1.0:
        e += 2e-5 + 6 * U * 1.0  # the quotient's 6 u through x^e, e <= 1
    if vignetting:
        e += 2.19e-5
    return e


def frame_variance_bound(accu, half, gamma=1.0, vignetting=False):
    """|v_float32 - v_float64| <= bound per channel, (H, W, 3): with dA, dB each within eps of their
    float64 values (display_error), the difference d = dA - dB is off by at most
    E = eps (dA + dB) + u |d| (one subtraction), its square by 2 |d| E + E^2 (+ one rounding), and the
    factor f (two products of rcp(w), two more) by 14 u; everything times (1 + 4 u) for the roundings
    left, plus the subnormal range."""
    A, B, f = display_halves_f64(accu, half, gamma, vignetting)
    eps = display_error(gamma, vignetting)
    d = np.abs(A - B)
    E = eps * (A + B) + U * d
    f3 = f[..., None]
    return ((2 * d * E + E * E) * f3 * (1 + 14 * U) + 16 * U * d * d * f3) * (1 + 4 * U) + 2.0 ** -126


def scalar_variance(var4, hit, m=None):
    """v_0 of the filter, (H, W) float64: v_r + v_g + v_b, demodulated sum_c v_c / m_c^2, 0 on a miss."""
    v = np.asarray(var4, np.float64)[..., :3]
    if m is not None:
        v = v / (np.asarray(m, np.float64) ** 2)
    return np.where(hit, v.sum(-1), 0.0)


# ----------------------------------------------------------------------------- the filter
def _frame_taps(H, W):
    yy, xx = np.mgrid[0:H, 0:W]

    def taps(face, ox, oy):
        qy, qx = yy + oy, xx + ox
        valid = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        return valid.reshape(-1), np.where(valid, qy * W + qx, 0).reshape(-1)
    return taps


def _cube_taps(W):
    def taps(face, ox, oy):
        valid, q = cref.tap_indices(W, face, ox, oy)
        return valid.reshape(-1), q.reshape(-1)
    return taps


def _filter(c, v, pos4, nrm4, faces, npix, taps, iterations, sigma_variance, variance_floor, sigma_normal,
            sigma_position):
    """Flat arrays over faces * npix pixels. Iteration i, step 2^i, the 25 taps, h, w_n, w_x, skip
    rules and centre weight of denoise_ref.atrous, and
      vbar_p = sum g v(q) / sum g over the 3x3 neighbours at distance 1, g = G3 x G3, taps off the
               surface or on a miss skipped, the centre always counted
      w_c    = exp(-|c_p - c_q|^2 / (sigma_variance^2 vbar_p + variance_floor))
      c'     = sum w c_q / sum w,   v' = sum w^2 v(q) / (sum w)^2     (centre: w = h(0)^2)
    sigma_variance^2 and variance_floor are the float32 values the library computes with."""
    sv2 = float(F(sigma_variance) * F(sigma_variance))
    floor = float(F(variance_floor))
    x = np.asarray(pos4, np.float64)[..., :3].reshape(-1, 3)
    t = np.asarray(pos4, np.float64)[..., 3].reshape(-1)
    n = np.asarray(nrm4, np.float64)[..., :3].reshape(-1, 3)
    hit = np.isfinite(t)
    c = c.reshape(-1, 3).copy()
    v = v.reshape(-1).copy()
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            cn, vn = c.copy(), v.copy()
            for f in range(faces):
                p = np.arange(f * npix, (f + 1) * npix)
                gv, gs = G3[1] * G3[1] * v[p], np.full(npix, G3[1] * G3[1])
                for ey in (-1, 0, 1):
                    for ex in (-1, 0, 1):
                        if ex == 0 and ey == 0:
                            continue
                        valid, q = taps(f, ex, ey)
                        ok = valid & hit[q]
                        g = G3[ex + 1] * G3[ey + 1]
                        gv = gv + np.where(ok, g * v[q], 0.0)
                        gs = gs + np.where(ok, g, 0.0)
                den = sv2 * (gv / gs) + floor
                num, wsum, vsum = np.zeros((npix, 3)), np.zeros(npix), np.zeros(npix)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        h = H5[dx + 2] * H5[dy + 2]
                        if dx == 0 and dy == 0:
                            w, q = np.full(npix, h), p
                        else:
                            valid, q = taps(f, dx * s, dy * s)
                            wn = np.maximum(0.0, (n[p] * n[q]).sum(-1)) ** sigma_normal
                            wx = np.exp(-np.abs((n[p] * (x[q] - x[p])).sum(-1)) / (sigma_position * t[p]))
                            wc = np.exp(-((c[p] - c[q]) ** 2).sum(-1) / den)
                            w = np.where(valid & hit[q], h * wn * wx * wc, 0.0)
                        w = np.where(hit[p], w, 0.0)
                        num += w[:, None] * c[q]
                        wsum += w
                        vsum += w * w * v[q]
                ph = hit[p]
                cn[p[ph]] = num[ph] / wsum[ph][:, None]
                vn[p[ph]] = vsum[ph] / wsum[ph] ** 2
            c, v = cn, vn
    return c, v


def atrous_var(c0, var4, pos4, nrm4, iterations, sigma_variance, variance_floor, sigma_normal, sigma_position,
               m=None, return_variance=False):
    """One frame: c0 (H, W, 3), var4 / pos4 / nrm4 (H, W, 4) -> the filtered frame (H, W, 3), float64.
    m (H, W, 3): the demodulated filter, on c0 / m with sum_c v_c / m_c^2, times m at the end."""
    c0 = np.asarray(c0, np.float64)
    H, W = c0.shape[:2]
    hit = np.isfinite(np.asarray(pos4)[..., 3])
    v0 = scalar_variance(var4, hit, m)
    if m is not None:
        c0 = c0 / m
    c, v = _filter(c0, v0, pos4, nrm4, 1, H * W, _frame_taps(H, W), iterations, sigma_variance, variance_floor,
                   sigma_normal, sigma_position)
    c = c.reshape(H, W, 3)
    if m is not None:
        c = c * m
    return (c, v.reshape(H, W)) if return_variance else c


def atrous_var_cube(c0, var4, pos4, nrm4, iterations, sigma_variance, variance_floor, sigma_normal, sigma_position):
    """One eye: c0 (6, W, W, 3), var4 / pos4 / nrm4 (6, W, W, 4), faces in cubeFaceIndex % 6 order;
    the 25 taps and the 3x3 variance neighbours that leave a face go through cube_tap (corner taps
    skipped)."""
    c0 = np.asarray(c0, np.float64)
    W = c0.shape[1]
    assert c0.shape == (6, W, W, 3)
    hit = np.isfinite(np.asarray(pos4)[..., 3])
    v0 = scalar_variance(var4, hit)
    c, _ = _filter(c0, v0, pos4, nrm4, 6, W * W, _cube_taps(W), iterations, sigma_variance, variance_floor,
                   sigma_normal, sigma_position)
    return c.reshape(6, W, W, 3)


def crosses_edge(W, iterations):
    """(W, W) bool: the pixels of a cube face one of whose 25 taps, in some iteration, or whose 3x3
    variance neighbours leave the face."""
    reach = max(1, 2 * (1 << (iterations - 1)))
    m = np.ones((W, W), bool)
    if W > 2 * reach:
        m[reach:W - reach, reach:W - reach] = False
    return m


def mse_ratios(frame, raw, conv):
    """(whole-frame, below-1) mean squared error of `frame` against conv over that of raw; below-1:
    the pixels whose largest channel is below 1 in both raw and conv."""
    frame, raw, conv = (np.asarray(a, np.float64) for a in (frame, raw, conv))
    dark = (conv.max(-1) < 1) & (raw.max(-1) < 1)
    whole = ((frame - conv) ** 2).mean() / ((raw - conv) ** 2).mean()
    below = ((frame - conv)[dark] ** 2).mean() / ((raw - conv)[dark] ** 2).mean()
    return float(whole), float(below)
