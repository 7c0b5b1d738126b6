"""float64 numpy restatement of the cube denoise ("cube"): the integer rule that says
where a filter tap lands when it leaves a face of the stereo cube, and the edge-avoiding a-trous
filter of tests/denoise_ref.py over the six faces of one eye with that rule. Written from the
definitions, not from the kernels."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from denoise_ref import H5

L, R, T, B = 0, 1, 2, 3
# (face, edge) -> (neighbour, the neighbour's edge the tap enters through, lateral index reversed)
TABLE = {
    0: {L: (3, R, False), R: (1, L, False), T: (4, T, True), B: (5, B, True)},
    1: {L: (0, R, False), R: (2, L, False), T: (4, L, False), B: (5, L, True)},
    2: {L: (1, R, False), R: (3, L, False), T: (4, B, False), B: (5, T, False)},
    3: {L: (2, R, False), R: (0, L, False), T: (4, R, True), B: (5, R, False)},
    4: {L: (1, T, False), R: (3, T, True), T: (0, T, True), B: (2, T, False)},
    5: {L: (1, B, True), R: (3, B, False), T: (2, B, False), B: (0, B, True)},
}


def cube_tap(W, face, qx, qy):
    """The tap (qx, qy) of face `face` (0..5) of W x W faces: (g, x, y), or None for a corner tap."""
    out_x, out_y = not 0 <= qx < W, not 0 <= qy < W
    if not out_x and not out_y:
        return face, qx, qy
    if out_x and out_y:
        return None
    if out_x:
        e, k, j = (L, -1 - qx, qy) if qx < 0 else (R, qx - W, qy)
    else:
        e, k, j = (T, -1 - qy, qx) if qy < 0 else (B, qy - W, qx)
    a = W * (2 * k + 1) // (2 * (W + 2 * k + 1))
    b = W * (k + j + 1) // (W + 2 * k + 1)
    g, e2, rev = TABLE[face][e]
    if rev:
        b = W - 1 - b
    return (g,) + {L: (a, b), R: (W - 1 - a, b), T: (b, a), B: (b, W - 1 - a)}[e2]


@lru_cache(maxsize=None)
def tap_indices(W, face, ox, oy):
    """For every pixel (y, x) of `face` the tap (x + ox, y + oy): (valid (W, W) bool, flat index
    (W, W) into a [6][W][W] array; 0 where not valid). Cached: the arrays are shared, not to be written."""
    valid = np.zeros((W, W), bool)
    idx = np.zeros((W, W), np.int64)
    for y in range(W):
        for x in range(W):
            t = cube_tap(W, face, x + ox, y + oy)
            if t is not None:
                valid[y, x] = True
                idx[y, x] = (t[0] * W + t[2]) * W + t[1]
    return valid, idx


def atrous_cube(c0, pos4, nrm4, iterations, sigma_color, sigma_normal, sigma_position):
    """One eye: c0 (6, W, W, 3), pos4 / nrm4 (6, W, W, 4), faces in cubeFaceIndex % 6 order -> the
    filtered faces (6, W, W, 3), float64. denoise_ref.atrous's weights; a tap that leaves its face
    reads the pixel cube_tap names, a corner tap or one that lands on a miss is skipped, the centre
    tap weighs h(0)^2 and a miss pixel keeps its value."""
    c = np.asarray(c0, np.float64).copy()
    F, W = c.shape[0], c.shape[1]
    assert c.shape == (6, W, W, 3)
    x = np.asarray(pos4, np.float64)[..., :3].reshape(-1, 3)
    t = np.asarray(pos4, np.float64)[..., 3].reshape(-1)
    n = np.asarray(nrm4, np.float64)[..., :3].reshape(-1, 3)
    hit = np.isfinite(t)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            sc = sigma_color / (1 << i) if sigma_color > 0 else 0.0
            cf = c.reshape(-1, 3)
            out = cf.copy()
            for f in range(F):
                p = np.arange(f * W * W, (f + 1) * W * W)
                num = np.zeros((W * W, 3))
                den = np.zeros(W * W)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        h = H5[dx + 2] * H5[dy + 2]
                        if dx == 0 and dy == 0:
                            w = np.full(W * W, h)
                            q = p
                        else:
                            valid, q = tap_indices(W, f, dx * s, dy * s)
                            valid, q = valid.reshape(-1), q.reshape(-1)
                            wn = np.maximum(0.0, (n[p] * n[q]).sum(-1)) ** sigma_normal
                            wx = np.exp(-np.abs((n[p] * (x[q] - x[p])).sum(-1)) / (sigma_position * t[p]))
                            w = h * wn * wx
                            if sc > 0:
                                w = w * np.exp(-((cf[p] - cf[q]) ** 2).sum(-1) / (sc * sc))
                            w = np.where(valid & hit[q], w, 0.0)
                        w = np.where(hit[p], w, 0.0)
                        num += w[:, None] * cf[q]
                        den += w
                ph = hit[p]
                out[p[ph]] = num[ph] / den[ph][:, None]
            c = out.reshape(c.shape)
    return c


def demodulated_atrous_cube(c0, pos4, nrm4, albedo4, iterations, power, floor, **weights):
    """atrous_cube on c0 / m, times m (denoise_albedo_ref.modulation), in float64."""
    from denoise_albedo_ref import modulation
    m = modulation(albedo4, power, floor)
    return atrous_cube(np.asarray(c0, np.float64) / m, pos4, nrm4, iterations, **weights) * m


# ----------------------------------------------------------------------------- geometry
def face_linear_maps(dirs, W):
    """L_f (3, 3) of one face from its camera-ray directions at the pixel centres (W * W, 3, row y,
    column x): dir is proportional to L_f (px, 1 - py, 1), px = (x + .5) / W. The directions are
    normalized, so the scale of each ray is eliminated by fitting L_f up to one factor: the null
    vector of the stacked cross-product equations dir x (L v) = 0."""
    c = (np.arange(W) + 0.5) / W
    px, py = np.meshgrid(c, c)
    v = np.stack([px.reshape(-1), 1 - py.reshape(-1), np.ones(W * W)], -1)  # (n, 3)
    d = np.asarray(dirs, np.float64)
    # dir x (L v) = 0 with L's 9 entries (row-major) unknown: [d]_x (I3 kron v^T) vec(L) = 0
    zero = np.zeros(len(d))
    dx = np.stack([np.stack([zero, -d[:, 2], d[:, 1]], -1), np.stack([d[:, 2], zero, -d[:, 0]], -1),
                   np.stack([-d[:, 1], d[:, 0], zero], -1)], 1)                    # (n, 3, 3)
    A = np.einsum("nij,nk->nijk", dx, v).reshape(-1, 9)
    _, sv, vt = np.linalg.svd(A, full_matrices=False)
    Lf = vt[-1].reshape(3, 3)
    if ((Lf @ v.T).T * d).sum() < 0:
        Lf = -Lf
    return Lf / np.linalg.norm(Lf), float(sv[-1] / sv[0])


def project(Lg, direction, W):
    """Continuous pixel coordinates (x, y) on the face with linear map Lg of a direction (the pixel
    that contains it is (floor x, floor y)); None behind the face."""
    v = np.linalg.solve(Lg, direction)
    if v[2] <= 0:
        return None
    return v[0] / v[2] * W, (1 - v[1] / v[2]) * W


# ----------------------------------------------------------------------------- the seam
def seam_pairs(W):
    """(p, q) flat indices into a [6][W][W] array: every pixel of a face's last column and the pixel
    the tap one step to its right lands on."""
    p, q = [], []
    for f in range(6):
        for y in range(W):
            g, x2, y2 = cube_tap(W, f, W, y)
            p.append((f * W + y) * W + W - 1)
            q.append((g * W + y2) * W + x2)
    return np.array(p), np.array(q)


def seam_error(c, conv, ok):
    """mean |(c(p) - c(q)) - (conv(p) - conv(q))| over seam_pairs whose two pixels both count (ok);
    c, conv (6, W, W, 3), ok (6, W, W)."""
    W = c.shape[1]
    p, q = seam_pairs(W)
    both = ok.reshape(-1)[p] & ok.reshape(-1)[q]
    cf, cv = np.asarray(c, np.float64).reshape(-1, 3), np.asarray(conv, np.float64).reshape(-1, 3)
    return float(np.abs((cf[p] - cf[q]) - (cv[p] - cv[q]))[both].mean())


def band_mse(c, conv, ok, b=1):
    """Mean squared error against conv over the counted pixels of every face's b-pixel border band."""
    W = c.shape[1]
    m = np.ones((W, W), bool)
    m[b:W - b, b:W - b] = False
    return float(((np.asarray(c, np.float64) - conv)[ok & m] ** 2).mean())


# ----------------------------------------------------------------------------- scene
def cube_args(size, spp):
    """Session arguments: the Cornell box seen from inside (eye (278, 273, 250), looking 25 degrees
    off +z, up (0, 1, 0)), -stereo, gamma 2.2. Every face of the cube has hits, the faces behind the
    eye also misses through the open front, and the cube's edges cross the walls mid-surface."""
    from pathlib import Path
    a = np.radians(25.0)
    scene = Path(__file__).resolve().parent.parent / "scenes" / "cornell_box.ecs"
    return ["-c", str(scene), "-vp", "278", "273", "250",
            "-vi", repr(278 + 100 * float(np.sin(a))), "273", repr(250 + 100 * float(np.cos(a))), "-vu", "0", "1", "0",
            "-size", str(size), str(size), "-spp", str(spp), "-gamma", "2.2", "-stereo"]
