"""float64 numpy restatement of the denoise stage and the scenes of
tests/test_denoise.py: the edge-avoiding a-trous filter, its 8-bit quantization and the tone
mapper's vignette. Written from the definitions, not from the kernels."""
from __future__ import annotations

import numpy as np

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)


def atrous(c0, pos4, nrm4, iterations, sigma_color, sigma_normal, sigma_position):
    """c0 (H, W, 3), pos4 / nrm4 (H, W, 4) -> the filtered frame (H, W, 3), float64.
    Iteration i: taps q = p + 2^i (dx, dy), dx, dy in -2..2, weight h(dx) h(dy) w_n w_x w_c with
      w_n = max(0, n_p . n_q) ^ sigma_normal
      w_x = exp(-|n_p . (x_q - x_p)| / (sigma_position t_p))
      w_c = exp(-|c_p - c_q|^2 / (sigma_color 2^-i)^2)      (sigma_color <= 0: 1)
    taps outside the image or on a miss (t = inf) are skipped, the centre tap weighs h(0)^2, and a
    miss pixel keeps its value."""
    c = np.asarray(c0, np.float64).copy()
    x = np.asarray(pos4, np.float64)[..., :3]
    t = np.asarray(pos4, np.float64)[..., 3]
    n = np.asarray(nrm4, np.float64)[..., :3]
    hit = np.isfinite(t)
    H, W = t.shape
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            sc = sigma_color / (1 << i) if sigma_color > 0 else 0.0
            num = np.zeros_like(c)
            den = np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    py = slice(max(0, -oy), min(H, H - oy))
                    px = slice(max(0, -ox), min(W, W - ox))
                    if py.start >= py.stop or px.start >= px.stop:
                        continue
                    qy = slice(py.start + oy, py.stop + oy)
                    qx = slice(px.start + ox, px.stop + ox)
                    h = H5[dx + 2] * H5[dy + 2]
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), h)
                    else:
                        wn = np.maximum(0.0, (n[py, px] * n[qy, qx]).sum(-1)) ** sigma_normal
                        wx = np.exp(-np.abs((n[py, px] * (x[qy, qx] - x[py, px])).sum(-1)) /
                                    (sigma_position * t[py, px]))
                        w = h * wn * wx
                        if sc > 0:
                            w = w * np.exp(-((c[py, px] - c[qy, qx]) ** 2).sum(-1) / (sc * sc))
                    w = np.where(hit[py, px] & hit[qy, qx], w, 0.0)
                    num[py, px] += w[..., None] * c[qy, qx]
                    den[py, px] += w
            out = c.copy()
            out[hit] = num[hit] / den[hit][:, None]
            c = out
    return c


def quantize(c):
    """(uint8)clamp(c * 255, 0, 255), the framebuffer's 8-bit store."""
    return np.clip(np.asarray(c, np.float64) * 255.0, 0.0, 255.0).astype(np.uint8)


def vignette(width, height):
    """DefaultToneMapper's factor cos(d / 2)^3, d = |(x, y) - (W, H) / 2| / (W / 2), (H, W) float64."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = np.hypot(xx - 0.5 * width, yy - 0.5 * height) / (0.5 * width)
    return np.cos(0.5 * d) ** 3


# ----------------------------------------------------------------------------- scenes
QUAD_NEAR_Z, QUAD_TILT_Z = 2.0, 4.0
# the quads' unit normals towards a camera at the origin looking along +z
N_NEAR = np.array([0.0, 0.0, -1.0])
N_TILT = np.array([-1.0, 0.0, -1.0]) / np.sqrt(2.0)


def two_quads():
    """[(positions, indices, cull)] of MeshScene: a quad facing a camera at the origin (looking along
    +z) at distance 2, x in [-1, 0.25], and one tilted 45 degrees about y through (1, 0, 4), x in
    [0, 2]: it covers the right half of the view behind the first. Small dyadic coordinates: the
    edge cross products are exact. Empty space above, below and to the left of both."""
    near = np.array([[-1, -0.5, 2], [0.25, -0.5, 2], [0.25, 0.5, 2], [-1, 0.5, 2]], np.float32)
    tilt = np.array([[0, -1.5, 5], [2, -1.5, 3], [2, 1.5, 3], [0, 1.5, 5]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return [(near, idx, False), (tilt, idx, False)]


def add_triangle_light(ms, v0=(-1.5, 2.5, -1.0), v1=(0.0, 2.5, 3.0), v2=(1.5, 2.5, -1.0), L=(30.0, 28.0, 24.0)):
    """An emissive triangle above a MeshScene's meshes and the camera (outside its view), facing down."""
    d = ms.dev
    tl = d.rtNewLight("trianglelight")
    for name, v in (("v0", v0), ("v1", v1), ("v2", v2), ("L", L)):
        d.rtSetFloat3(tl, name, *v)
    d.rtCommit(tl)
    d.rtSetPrimitive(ms.scene, 2, d.rtNewLightPrimitive(tl))
    d.rtCommit(ms.scene)


def sphere_mesh(num_theta, num_phi, r=1.0, centre=(0.0, 0.0, 0.0), step=0.001):
    """The sphere shape's mesh (shapes/sphere.h) in float64: vertices r * e(theta, phi) + centre with
    e = (sin t cos p, cos t, sin t sin p), vertex normals normalize(cross(dpdv, dpdu)) of the
    forward differences over `step` grid units, two triangles per cell. Returns (positions (n, 3),
    normals (n, 3), triangles (m, 3), sin(theta) per vertex)."""
    def e(t, p):
        return np.stack([np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)], -1)

    th, ph = np.meshgrid(np.arange(num_theta + 1, dtype=np.float64), np.arange(num_phi, dtype=np.float64),
                         indexing="ij")
    a, b = np.pi / num_theta, 2 * np.pi / num_phi
    p = e(th * a, ph * b)
    dpdu = e((th + step) * a, ph * b) - p
    dpdv = e(th * a, (ph + step) * b) - p
    with np.errstate(all="ignore"):
        nrm = np.cross(dpdv, dpdu)
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    tris = []
    for t in range(1, num_theta + 1):
        for f in range(1, num_phi + 1):
            p00, p01 = (t - 1) * num_phi + f - 1, (t - 1) * num_phi + f % num_phi
            p10, p11 = t * num_phi + f - 1, t * num_phi + f % num_phi
            if t > 1:
                tris.append((p10, p00, p01))
            if t < num_theta:
                tris.append((p11, p10, p01))
    pos = (r * p + np.asarray(centre, np.float64)).reshape(-1, 3)
    return pos, nrm.reshape(-1, 3), np.array(tris), np.sin(th * a).reshape(-1)
