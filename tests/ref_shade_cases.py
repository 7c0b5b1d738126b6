"""Inputs of the shading-layer pin (tests/test_ref_shade.py, tests/golden/make_ref_shade.py).

Every case has ROWS rows: hand-written edge rows first, then random rows from a fixed seed. The
inputs are regenerated from this module on every run; the fixtures hold the reference library's
outputs and a checksum of the inputs they belong to (`digest`), so a drift of the generator is an
assertion, not a silent mismatch.

BRDF rows carry the constructor arguments of the reference class of each CompKind
(kernels/yrt_shade.h:36-55) as args[16] = R.rgb, p0, p1, p2, eta.rgb, k.rgb, pad.
"""
import hashlib
import struct

import numpy as np

ROWS = 1024
F = np.float32
ONE_M = np.nextafter(F(1), F(0))  # the largest float below 1
TINY = np.nextafter(F(0), F(1))   # 1 ulp above 0 (subnormal)
MINN = F(1.1754944e-38)           # the smallest normal

KIND_NAMES = ["lambert", "diel_refl", "const_diel_trans", "thin_diel_trans", "diel_layer_lamb", "microfacet",
              "transmission", "specular", "reflection", "conductor", "micro_cond", "micro_aniso", "minnaert",
              "velvety", "diel_trans", "diel_layer_glitter"]

# (etai, etat): eta_ = 1/1.5, 1.5 (with rows past the critical angle) and 1. eta_ = 1 makes the
# dielectric reflection's colour zero and eta_ = 1.5 past the critical angle a transmission's pdf
# zero, both rejected samples: they get one and two variants in eight.
ETAS = [(1.0, 1.5), (1.5, 1.0), (1.0, 1.5), (1.0, 1.5), (1.0, 1.0), (1.0, 1.5), (1.5, 1.0), (1.0, 1.5)]
# exponents {0, 1, 64, 1e4}, and 1 / roughness for roughness {1e-3, 0.5}; a microfacet sample at a
# low exponent often lands below the horizon (rejected), so the high ones come more often
EXPS = [0.0, 64.0, 1.0, 1e4, 1e3, 2.0, 64.0, 1e4, 1e3, 64.0, 256.0, 1e3]
# Minnaert's and Velvety's colour is pow(cosine or sine, exponent): zero at the high exponents for
# most directions (a rejected sample), so those come once in twelve each
SOFT_EXPS = [0.0, 1.0, 0.5, 64.0, 2.0, 1.0, 3.0, 1e4, 0.0, 2.0, 1.0, 0.5]


def cpu_vendor():
    """vendor_id of /proc/cpuinfo: rcpps / rsqrtps tables are vendor-specific, the fixtures Intel's."""
    from pathlib import Path
    for line in Path("/proc/cpuinfo").read_text().splitlines():
        if line.startswith("vendor_id"):
            return line.split(":", 1)[1].strip()
    return "?"


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint64).copy()


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _frames(rng, n):
    """Ns, Ng (within ~15 degrees of Ns), and an orthonormal tangent pair of Ns."""
    Ns = _unit(rng.standard_normal((n, 3)))
    Ng = _unit(Ns + 0.15 * rng.standard_normal((n, 3)))
    t = rng.standard_normal((n, 3))
    Tx = _unit(t - Ns * (t * Ns.astype(np.float64)).sum(-1, keepdims=True))
    Ty = np.cross(Ns.astype(np.float64), Tx.astype(np.float64)).astype(F)
    return Ns, Ng, Tx, Ty


def _reflect(wo, N):
    d = (wo * N).sum(-1, keepdims=True, dtype=F)
    return (F(2) * d * N - wo).astype(F)


def brdf_directions(seed):
    """wo, Ns, Ng, Tx, Ty, wi (ROWS, 3), s (ROWS, 2), ss (ROWS)."""
    rng = np.random.default_rng(seed)
    n = ROWS
    Ns, Ng, Tx, Ty = _frames(rng, n)
    # wo from the whole sphere, drawn towards Ns by a random weight (grazing directions included);
    # all but three rows in a hundred see the surface from above Ns (a sample from below is rejected)
    wo = _unit(rng.standard_normal((n, 3)) + Ns * (4.0 * rng.random((n, 1))))
    flip = ((wo * Ns).sum(-1) < 0) & (rng.random(n) < 0.97)
    wo[flip] = -wo[flip]
    wi = _unit(rng.standard_normal((n, 3)))
    up = ((wi * Ns).sum(-1) < 0) & (rng.random(n) < 0.7)
    wi[up] = -wi[up]
    s = rng.random((n, 2), dtype=F)
    ss = rng.random(n, dtype=F)
    k = n // 8
    wi[n - k:] = _reflect(wo[n - k:], Ns[n - k:])  # wi == reflect(wo)
    # ---- edge rows: the frame Ns = z, Tx = x, Ty = y
    e = []
    z, ng2 = (0, 0, 1), tuple(_unit([0.6, 0, 0.8]))
    generic_wo, generic_wi = tuple(_unit([0.3, -0.2, 0.9])), tuple(_unit([-0.5, 0.4, 0.7]))

    def row(wo_, wi_, s_=(0.37, 0.61), ss_=0.42, Ng_=z):
        e.append((wo_, z, Ng_, (1, 0, 0), (0, 1, 0), wi_, s_, ss_))

    for zc in (0.0, float(TINY), -float(TINY), float(MINN), -float(MINN)):  # wo.Ns in {0, +-1 ulp}
        row((1.0, 0.0, zc), generic_wi)
        row((0.6, 0.8, zc), (-0.6, -0.8, 0.0))
    row(z, generic_wi)                                   # wo.Ns = 1
    row(z, z)
    row((0.6, 0.0, -0.8), generic_wi)                    # wo below the horizon
    row((0.0, -0.6, -0.8), (0.0, 0.6, 0.8))
    row(generic_wo, tuple(_unit([-0.9, 0, 0.436])), Ng_=ng2)   # wi above Ns, below Ng
    row(generic_wo, tuple(_unit([0.9, 0, -0.2])), Ng_=ng2)     # wi below Ns, above Ng
    row(generic_wo, tuple(_reflect(np.array([generic_wo], F), np.array([z], F))[0]))  # wi == reflect(wo)
    row((0.6, 0.0, 0.8), (-0.6, 0.0, 0.8))
    for a in (0.0, 0.5, float(ONE_M)):                   # s and ss in {0, 0.5, 1 - ulp}
        for b in (0.0, 0.5, float(ONE_M)):
            for c in (0.0, 0.5, float(ONE_M)):
                row(generic_wo, generic_wi, (a, b), c)
    grazing = tuple(_unit([0.999, 0, 0.04]))             # past the critical angle for eta_ = 1.5
    for a in (0.1, 0.5, 0.9):
        row(grazing, generic_wi, (a, 0.5))
    m = len(e)
    for i, (a, b, c, d, f, g, h, j) in enumerate(e):
        wo[i], Ns[i], Ng[i], Tx[i], Ty[i], wi[i], s[i], ss[i] = a, b, c, d, f, g, h, j
    return dict(wo=wo, Ns=Ns, Ng=Ng, Tx=Tx, Ty=Ty, wi=wi, s=s, ss=ss, edge_rows=m)


def brdf_args(kind, seed):
    """(ROWS, 16) constructor arguments of component `kind`; row i takes variant i of each cycle."""
    rng = np.random.default_rng(1000 + 17 * kind + seed)
    n = ROWS
    a = np.zeros((n, 16), F)
    i = np.arange(n)
    a[:, 0:3] = rng.random((n, 3), dtype=F)
    a[i % 7 == 3, 1] = 0.0                       # R = 0 in one channel
    a[:, 6:9] = (0.1 + 4.9 * rng.random((n, 3))).astype(F)   # conductor eta
    a[:, 9:12] = (5.0 * rng.random((n, 3))).astype(F)        # conductor k
    a[i % 5 == 2, 9:12] = 0.0                    # k = 0
    eta = np.array(ETAS, F)[i % len(ETAS)]
    exps = np.array(EXPS, F)[(i // 2) % len(EXPS)]
    if kind in (1, 3, 4, 5, 14, 15):
        a[:, 3:5] = eta
    if kind == 1:
        a[:, 5] = np.array([1.0, 0.25], F)[i % 2]            # alpha
    elif kind == 2:
        a[:, 3] = rng.random(n, dtype=F)                     # opacity
    elif kind == 3:
        a[:, 0:3] = np.maximum(a[:, 0:3], F(0.05))           # T > 0 (log T)
        a[:, 5] = np.array([0.1, 1.0, 3.0], F)[i % 3]        # thickness
    elif kind in (5, 15):
        a[:, 5] = exps
    elif kind in (7, 10):
        a[:, 3] = exps
    elif kind in (12, 13):
        a[:, 3] = np.array(SOFT_EXPS, F)[i % len(SOFT_EXPS)]
    elif kind == 11:
        a[:, 3] = exps
        a[:, 4] = np.array(EXPS, F)[(i // 3) % len(EXPS)]
    return a


def brdf_case(kind):
    d = brdf_directions(100 + kind)
    d["args"] = brdf_args(kind, 0)
    if kind in (4, 15):
        # a dielectric layer over eta 1.5 reflects a ground sample back inside when its cosine is
        # below 0.745 (pdf 0, rejected): more than half of all cosine-weighted samples. The random
        # rows draw s.y from [0.5, 1) (the glitter's half vector: [0.8, 1)) so that most leave the
        # layer; the edge rows keep theirs.
        m, lo = d["edge_rows"], F(0.5 if kind == 4 else 0.8)
        d["s"][m:, 1] = lo + (F(1) - lo) * d["s"][m:, 1]
    return d


# component sets the materials create (materials/*.h): name -> kinds in the order they are added
SETS = {
    "matte": [0], "metallicpaint": [1, 4], "metallicpaint_glitter": [1, 4, 15], "obj": [6, 0, 7],
    "uber_refl": [0, 2, 1], "uber_rough": [0, 2, 5], "uber_opaque": [0, 5], "thindielectric": [1, 3],
    "plastic": [4, 1], "plastic_rough": [4, 5], "dielectric": [1, 14], "mirror": [8], "metal": [9],
    "metal_rough": [10], "brushedmetal": [11], "velvet": [12, 13],
}


def set_case(name):
    kinds = SETS[name]
    d = brdf_directions(300 + sorted(SETS).index(name))
    d["args"] = np.stack([brdf_args(k, 50 + j) for j, k in enumerate(kinds)], 1)
    d["frame"] = np.concatenate([d["Ns"], d["Ng"], d["Tx"], d["Ty"]], 1)
    d["kinds"] = np.array(kinds, np.int32)
    return d


def rejected(color, pdf):
    """CompositedBRDF's own rule (compositedbrdf.h:129): colour all zero, or pdf <= 0."""
    return (color == 0).all(-1) | (pdf <= 0)


# ---------------------------------------------------------------- cameras
CAM_FIELDS = ["local2world", "angle", "aspectRatio", "lensRadius", "focalDistance", "cubeFaceIndex", "toeIn",
              "eyeSeparation", "zeroParallaxDistance", "stereFalloffAngle", "sceneScale", "origin", "lookAt", "up"]
_CAM_AT = {"local2world": 0, "angle": 12, "aspectRatio": 13, "lensRadius": 14, "focalDistance": 15,
           "cubeFaceIndex": 16, "toeIn": 17, "eyeSeparation": 18, "zeroParallaxDistance": 19, "stereFalloffAngle": 20,
           "sceneScale": 21, "origin": 22, "lookAt": 25, "up": 28}
_CAM_VT = {"local2world": 16, "cubeFaceIndex": 8, "toeIn": 1, "origin": 11, "lookAt": 11, "up": 11}  # else FLOAT1 = 9
CAM_KIND = {"pinhole": 0, "depthoffield": 1, "stereo": 2}


def look_at(eye, point, up):
    """AffineSpace3f::lookAtPoint's layout (vx, vy, vz, p), in float32 numpy: any rigid frame will do."""
    eye, point, up = (np.asarray(x, np.float64) for x in (eye, point, up))
    z = (point - eye) / np.linalg.norm(point - eye)
    u = np.cross(up, z)
    u /= np.linalg.norm(u)
    v = np.cross(z, u)
    return np.concatenate([u, v, z, eye]).astype(F)


def camera_params(parms):
    """The float32[32] record oracle/ref_shade.cpp reads: the fields present, and their mask."""
    p = np.zeros(32, F)
    mask = 0
    for k, v in parms.items():
        v = np.atleast_1d(np.asarray(v, F))
        p[_CAM_AT[k]:_CAM_AT[k] + v.size] = v
        mask |= 1 << CAM_FIELDS.index(k)
    p[31] = F(mask)
    return p


def camera_blob(typ, parms):
    """A frame blob (device/export.cpp's format) holding nothing but this camera."""
    def s(x):
        b = x.encode()
        return struct.pack("<I", len(b)) + b
    out = b"YRTF" + struct.pack("<II", 1, 1) + struct.pack("<I", 0) + s(typ) + struct.pack("<I", len(parms))
    for k, v in parms.items():
        vt = _CAM_VT.get(k, 9)
        out += s(k) + struct.pack("<I", vt)
        v = np.atleast_1d(np.asarray(v, F))
        if vt == 16:
            out += v.astype("<f4").tobytes()
        elif vt in (1, 8):
            out += struct.pack("<4i", int(v[0]), 0, 0, 0)
        else:
            out += np.concatenate([v, np.zeros(4 - v.size, F)]).astype("<f4").tobytes()
    return out + struct.pack("<IiiI", 0, -1, 0, 0)


def _pixels(seed):
    rng = np.random.default_rng(seed)
    px = rng.random((ROWS, 2), dtype=F)
    lens = rng.random((ROWS, 2), dtype=F)
    e = [(.5, .5), (0, 0), (1, 0), (0, 1), (1, 1), (float(ONE_M), float(ONE_M)), (.5, 0), (.5, 1), (0, .5), (1, .5),
         (.5, .25), (.5, .75), (.25, .5), (.75, .5), (.5, float(np.nextafter(F(.5), F(1)))),
         (float(np.nextafter(F(.5), F(0))), .5)]
    px[:len(e)] = np.array(e, F)
    px[len(e):64, 0] = 0.5            # exactly 0.5 on one axis (the poles of faces 4 and 5)
    px[64:112, 1] = 0.5
    # the lens sample at the centre (r = 0) and on the rim (r = 1 - ulp), at several angles
    lens[:8] = np.array([(0, 0), (0, .5), (float(ONE_M), 0), (float(ONE_M), .25), (float(ONE_M), .5),
                         (float(ONE_M), .75), (float(ONE_M), float(ONE_M)), (.5, .5)], F)
    lens[112:128, 0] = 0.0
    lens[128:144, 0] = ONE_M
    return px, lens


def camera_cases():
    """name -> (type, parms, pixel (ROWS, 2), lens (ROWS, 2))"""
    l2w = look_at((2.25, 8.25, -0.05), (3.15, 7.8, -0.05), (0.4365, 0.8997, -0.0029))
    l2w_c1 = look_at((278, 273, -800), (278, 273, 0), (0, 1, 0))
    cases = {}
    for face in range(12):
        for toe in (0, 1):
            parms = {"local2world": l2w, "cubeFaceIndex": face, "toeIn": toe,
                     "stereFalloffAngle": [0.0, 30.0, 90.0][(face + toe) % 3], "origin": l2w[9:12],
                     "up": (0.0, 1.0, 0.0)}
            if face % 4 == 1:
                parms.update(lookAt=(3.15, 7.8, -0.05), eyeSeparation=0.3, zeroParallaxDistance=4.0, sceneScale=2.0)
            cases[f"stereo_f{face}_toe{toe}"] = ("stereo", parms, *_pixels(500 + 2 * face + toe))
    # a zero parallax distance of 0 disables toe-in (StereoCubeCamera.h:32-39); class defaults otherwise
    cases["stereo_zpd0"] = ("stereo", {"local2world": l2w_c1, "cubeFaceIndex": 7, "toeIn": 1,
                                       "zeroParallaxDistance": 0.0}, *_pixels(540))
    cases["stereo_defaults"] = ("stereo", {"local2world": l2w_c1}, *_pixels(541))
    cases["pinhole_c3"] = ("pinhole", {"local2world": l2w, "angle": 60.0, "aspectRatio": 1.5}, *_pixels(542))
    cases["pinhole_defaults"] = ("pinhole", {"local2world": l2w_c1}, *_pixels(543))
    cases["dof"] = ("depthoffield", {"local2world": l2w, "angle": 45.0, "aspectRatio": 1.25, "lensRadius": 0.05,
                                    "focalDistance": 3.0}, *_pixels(544))
    cases["dof_big_lens"] = ("depthoffield", {"local2world": l2w_c1, "lensRadius": 25.0, "focalDistance": 800.0},
                             *_pixels(545))
    return cases


# ---------------------------------------------------------------- the three implementations
def _p(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def ref_brdf(lib, kind, c):
    """oracle/_ref/libref_shade.so's ref_brdf on a brdf_case: eval, sample, wi (ROWS, 3), pdf."""
    n = c["args"].shape[0]
    ev, sa, wi = (np.zeros((n, 3), F) for _ in range(3))
    pdf = np.zeros(n, F)
    rc = lib.ref_brdf(kind, _p(c["args"]), n, *[_p(c[k]) for k in ("wo", "Ns", "Ng", "Tx", "Ty", "wi", "s")],
                      _p(ev), _p(sa), _p(wi), _p(pdf))
    assert rc == 0
    return ev, sa, wi, pdf


def oracle_brdf(kind, c):
    import oracle
    return oracle.brdf(kind, *[c[k] for k in ("args", "wo", "Ns", "Ng", "Tx", "Ty", "wi", "s")])


def ref_set_sample(lib, c):
    n = c["args"].shape[0]
    col, wi = np.zeros((n, 3), F), np.zeros((n, 3), F)
    pdf, typ = np.zeros(n, F), np.zeros(n, np.uint32)
    rc = lib.ref_brdf_set_sample(len(c["kinds"]), _p(c["kinds"]), _p(c["args"]), n,
                                 *[_p(c[k]) for k in ("wo", "frame", "s", "ss")], _p(col), _p(wi), _p(pdf), _p(typ))
    assert rc == 0
    return col, wi, pdf, typ


def oracle_set_sample(c):
    import oracle
    return oracle.brdf_set_sample(*[c[k] for k in ("kinds", "args", "wo", "frame", "s", "ss")])


def ref_camera(lib, typ, parms, px, lens):
    org, dir_ = np.zeros((px.shape[0], 3), F), np.zeros((px.shape[0], 3), F)
    p = camera_params(parms)
    assert lib.ref_camera_rays(CAM_KIND[typ], _p(p), px.shape[0], _p(px), _p(lens), _p(org), _p(dir_)) == 0
    return org, dir_


def oracle_camera(typ, parms, px, lens):
    import oracle
    return oracle.camera_rays_lens(camera_blob(typ, parms), px, lens)


def same_bits(a, b):
    """Rows whose words are bit-identical; a NaN equals any NaN (the sign and payload
    of a generated NaN belong to the instruction set, x86 SSE makes 0xffc00000, gfx950 0x7fc00000)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return ok.reshape(a.shape[0], int(np.prod(a.shape[1:]))).all(1)


# ---------------------------------------------------------------- lights
LIGHT_KIND = {"trianglelight": 1, "pointlight": 3, "spotlight": 4, "directionallight": 5, "distantlight": 6}
_ID = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
# a rotation about (1, 2, 3) scaled by 1.5, then a translation: Light::transform does not
# renormalize a spot light's direction (spotlight.h:33-39)
_c, _s = np.cos(0.7), np.sin(0.7)
_u = np.array([1, 2, 3]) / np.sqrt(14.0)
_R = 1.5 * (_c * np.eye(3) + _s * np.array([[0, -_u[2], _u[1]], [_u[2], 0, -_u[0]], [-_u[1], _u[0], 0]]) +
            (1 - _c) * np.outer(_u, _u))
_XF = np.concatenate([_R.T.ravel(), [3.0, -2.0, 5.0]]).astype(F)  # columns vx, vy, vz, then p


def light_params(xfm, parms):
    p = np.zeros(32, F)
    p[0:12] = xfm
    for key, at in (("P", 12), ("v0", 12), ("D", 15), ("v1", 15), ("v2", 18), ("I", 21), ("E", 21), ("L", 21),
                    ("angleMin", 24), ("halfAngle", 24), ("angleMax", 25)):
        if key in parms:
            v = np.atleast_1d(np.asarray(parms[key], F))
            p[at:at + v.size] = v
    return p


def light_blob(typ, parms):
    """A frame blob holding nothing but this light object."""
    def s(x):
        b = x.encode()
        return struct.pack("<I", len(b)) + b
    out = b"YRTF" + struct.pack("<II", 1, 1) + struct.pack("<I", 6) + s(typ) + struct.pack("<I", len(parms))
    for k, v in parms.items():
        v = np.atleast_1d(np.asarray(v, F))
        out += s(k) + struct.pack("<I", 11 if v.size == 3 else 9)
        out += np.concatenate([v, np.zeros(4 - v.size, F)]).astype("<f4").tobytes()
    return out + struct.pack("<IiiI", 0, -1, -1, 0)


def _light_rows(seed, xfm, parms, toward=(0, -1, 0)):
    """P (ROWS, 3) and s (ROWS, 2): points about the placed light over many distances, then the
    edge rows: on the light's axis, inside, between and outside a spot's two cones, at the light's
    position, and the triangle samples at the three corners."""
    rng = np.random.default_rng(seed)
    n = ROWS
    M, t = xfm[:9].astype(np.float64).reshape(3, 3).T, xfm[9:12].astype(np.float64)
    pos = M @ np.asarray(parms.get("P", parms.get("v0", (0, 0, 0))), np.float64) + t
    P = pos + rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 1))
    s = rng.random((n, 2), dtype=F)
    D = np.asarray(parms.get("D", toward), np.float64)  # a triangle light: its lit side
    axis = M @ (D / np.linalg.norm(D))
    axis /= np.linalg.norm(axis)
    perp = np.cross(axis, [0.3, 0.5, 0.8])
    perp /= np.linalg.norm(perp)
    # the second half of the random rows lies within 30 degrees of the axis (a spot's cones)
    h = n // 2
    ang, turn = np.deg2rad(30.0) * rng.random((h, 1)), 2 * np.pi * rng.random((h, 1))
    side = np.cos(turn) * perp + np.sin(turn) * np.cross(axis, perp)
    P[h:] = pos + 10.0 ** rng.uniform(-3, 3, (h, 1)) * (np.cos(ang) * axis + np.sin(ang) * side)
    k = 0
    for deg in (0.0, 5.0, 10.0, 12.0, 15.0, 18.0, 20.0, 25.0, 60.0, 90.0, 120.0, 180.0):
        for dist in (1e-3, 1.0, 250.0):
            a = np.deg2rad(deg)
            P[k] = pos + dist * (np.cos(a) * axis + np.sin(a) * perp)
            k += 1
    P = P.astype(F)
    P[k] = pos.astype(F)      # at the light's position, as exactly as float32 holds it
    P[k + 1] = (M.astype(F) @ np.asarray(parms.get("P", parms.get("v0", (0, 0, 0))), F)) + xfm[9:12]
    k += 2
    for c in ((0, 0), (0, .5), (float(ONE_M), 0), (float(ONE_M), float(ONE_M)), (1, 0), (1, 1), (.25, .5), (.5, .5)):
        s[k] = c              # triangle samples at the corners v0, v2, v1 (and the cone's axis and rim)
        k += 1
    return P, s


def light_cases():
    """name -> (type, parms, xfm12, P, s)"""
    protos = {
        "point": ("pointlight", {"P": (1.0, 2.0, -0.5), "I": (10.0, 8.0, 0.0)}),
        "spot": ("spotlight", {"P": (1.0, 2.0, -0.5), "D": (0.2, -1.0, 0.3), "I": (10.0, 8.0, 6.0), "angleMin": 20.0,
                               "angleMax": 40.0}),
        "spot_hard": ("spotlight", {"P": (0.0, 4.0, 0.0), "D": (0.0, -2.0, 0.0), "I": (3.0, 3.0, 3.0),
                                    "angleMin": 30.0, "angleMax": 30.0}),
        "directional": ("directionallight", {"D": (0.2, -1.0, 0.3), "E": (2.0, 1.0, 0.5)}),
        "distant": ("distantlight", {"D": (0.2, -1.0, 0.3), "L": (2.0, 1.0, 0.5), "halfAngle": 5.0}),
        "distant_wide": ("distantlight", {"D": (0.0, 0.0, -3.0), "L": (1.0, 1.0, 1.0), "halfAngle": 90.0}),
        "triangle": ("trianglelight", {"v0": (-1.0, 3.0, -1.0), "v1": (1.0, 3.0, -1.0), "v2": (0.0, 3.0, 1.5),
                                       "L": (15.0, 15.0, 12.0)}),
    }
    cases = {}
    for j, (name, (typ, parms)) in enumerate(protos.items()):
        for xn, xfm in (("id", _ID), ("xfm", _XF)):
            if xn == "xfm" and name in ("spot_hard", "distant_wide"):
                continue
            cases[f"{name}_{xn}"] = (typ, parms, xfm, *_light_rows(700 + 2 * j + (xn == "xfm"), xfm, parms, (0, 1, 0)))
    return cases


def ref_light(lib, typ, parms, xfm, P, s):
    n = P.shape[0]
    L, wi, pdf = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros(n, F)
    p = light_params(xfm, parms)
    assert lib.ref_light_sample(LIGHT_KIND[typ], _p(p), n, _p(P), _p(s), _p(L), _p(wi), _p(pdf)) == 0
    return L, wi, pdf


def oracle_light(typ, parms, xfm, P, s):
    import oracle
    Ns = np.tile(np.array([0, 0, 1], F), (P.shape[0], 1))
    return oracle.light_sample(light_blob(typ, parms), xfm, P, Ns, s)


# ---------------------------------------------------------------- the filtered sample table
# (spp, iteration, num1D, num2D) at 64 sets: the shapes of test_sample_tables_without_filter
TABLE_SHAPES = [(1, 0, 2, 3), (16, 0, 2, 3), (64, 0, 10, 11), (256, 0, 10, 11), (16, 5, 2, 3), (64, 3, 10, 11)]
# the tables of progressive frames (rtRenderFrame(..., accumulate=1), tests/test_progressive.py): the
# last iteration of a 64-sample chunk, the first and the second of the next one (spp 1: 63, 64, 65;
# spp 16: 3, 4), and an spp the factory rounds up to a power of two (3 -> 4, offset 20)
TABLE_SHAPES += [(1, 63, 2, 3), (1, 64, 2, 3), (1, 65, 2, 3), (16, 3, 2, 3), (16, 4, 2, 3), (3, 5, 2, 3)]


def pow2_spp(spp):
    """SamplerFactory's samplesPerPixel: spp rounded up to a power of two (samplers/sampler.cpp:91)."""
    p = 1
    while p < spp:
        p <<= 1
    return p


def ref_sample_table(lib, spp, sets, iteration, n1, n2, bspline):
    """The reference's own SamplerFactory::init table (dims, sets * pow2_spp(spp))."""
    rec = sets * pow2_spp(spp)
    out = np.zeros((5 + n1 + 2 * n2, rec), F)
    assert lib.ref_sample_table(spp, sets, iteration, n1, n2, int(bool(bspline)), _p(out)) == rec
    return out


# ---------------------------------------------------------------- materials
VACUUM = (1.0, 1.0, 1.0, 1.0)
# name -> (class, Parms, current medium): the parameter sets of scenes/materials_lights.xml, each
# material's defaults, and the branches the constructors' parameters choose between
MATERIALS = {
    "matte_scene": ("Matte", {"reflectance": (0.6, 0.5, 0.4)}, VACUUM),
    "matte_default": ("Matte", {}, VACUUM),
    "plastic_scene": ("Plastic", {"pigmentColor": (0.8, 0.1, 0.1), "roughness": 0.05}, VACUUM),
    "plastic_smooth": ("Plastic", {"pigmentColor": (0.1, 0.6, 0.1), "roughness": 0.0}, VACUUM),
    "plastic_default": ("Plastic", {}, VACUUM),
    "dielectric_scene_outside": ("Dielectric", {"etaInside": 1.5, "transmission": (0.9, 0.95, 0.99)}, VACUUM),
    "dielectric_scene_inside": ("Dielectric", {"etaInside": 1.5, "transmission": (0.9, 0.95, 0.99)},
                                (0.9, 0.95, 0.99, 1.5)),
    "dielectric_default": ("Dielectric", {}, VACUUM),
    "mirror_scene": ("Mirror", {"reflectance": (0.9, 0.9, 0.9)}, VACUUM),
    "mirror_default": ("Mirror", {}, VACUUM),
    "metal_scene": ("Metal", {"eta": (0.2, 0.4, 1.4), "k": (3.0, 2.6, 2.0), "roughness": 0.1}, VACUUM),
    "metal_smooth": ("Metal", {"reflectance": (0.95, 0.8, 0.6), "roughness": 0.0}, VACUUM),
    "metal_default": ("Metal", {}, VACUUM),
    "brushedmetal_scene": ("BrushedMetal", {"eta": (0.3, 0.3, 0.3), "k": (2.5, 2.5, 2.5), "roughnessX": 0.05,
                                            "roughnessY": 0.4}, VACUUM),
    "brushedmetal_smooth": ("BrushedMetal", {"roughnessX": 0.0, "roughnessY": 0.4}, VACUUM),
    "brushedmetal_default": ("BrushedMetal", {}, VACUUM),
    "velvet_scene": ("Velvet", {"reflectance": (0.5, 0.3, 0.6), "backScattering": 0.5,
                                "horizonScatteringColor": (0.8, 0.8, 0.9), "horizonScatteringFallOff": 2.0}, VACUUM),
    "velvet_default": ("Velvet", {}, VACUUM),
    "metallicpaint": ("MetallicPaint", {"shadeColor": (0.7, 0.1, 0.1), "eta": 1.45}, VACUUM),
    "metallicpaint_glitter": ("MetallicPaint", {"shadeColor": (0.1, 0.2, 0.7), "glitterColor": (0.9, 0.9, 0.8),
                                                "glitterSpread": 0.05, "eta": 1.45}, VACUUM),
    "metallicpaint_default": ("MetallicPaint", {}, VACUUM),
    "thindielectric": ("ThinDielectric", {"transmission": (0.9, 0.6, 0.3), "eta": 1.5, "thickness": 0.4,
                                          "transparency": 0.8}, VACUUM),
    "thindielectric_default": ("ThinDielectric", {}, VACUUM),
}


def material_rows(name):
    """(ROWS, 20) = wo, Ns, Ng, Tx, Ty, wi, s. One row feeds every component the material creates, so
    the random rows are shaped for the most demanding of them, as brdf_case does for kinds 4 and 15:
    a dielectric layer (Plastic, MetallicPaint) sends a ground sample back inside when its cosine
    is below 0.745, and a ray inside glass (Dielectric seen from inside) is totally reflected when
    cos(wo, Ns) is below 0.745; both are rejected samples. s.y comes from [0.8, 1) and a wo above
    the surface is pulled towards Ns (cos(wo, Ns) >= 0.83). The edge rows keep their values."""
    d = brdf_directions(900 + sorted(MATERIALS).index(name))
    m = d["edge_rows"]
    d["s"][m:, 1] = F(0.8) + F(0.2) * d["s"][m:, 1]
    wo, Ns = d["wo"][m:].astype(np.float64), d["Ns"][m:].astype(np.float64)
    above = (wo * Ns).sum(-1, keepdims=True) > 0
    d["wo"][m:] = np.where(above, _unit(wo + 1.5 * Ns), d["wo"][m:])
    return np.concatenate([d[k] for k in ("wo", "Ns", "Ng", "Tx", "Ty", "wi", "s")], 1)


def material_blob(typ, parms):
    def s(x):
        b = x.encode()
        return struct.pack("<I", len(b)) + b
    out = b"YRTF" + struct.pack("<II", 1, 1) + struct.pack("<I", 4) + s(typ) + struct.pack("<I", len(parms))
    for k, v in parms.items():
        v = np.atleast_1d(np.asarray(v, F))
        out += s(k) + struct.pack("<I", 11 if v.size == 3 else 9)
        out += np.concatenate([v, np.zeros(4 - v.size, F)]).astype("<f4").tobytes()
    return out + struct.pack("<IiiI", 0, -1, -1, 0)


def ref_material(lib, typ, parms, medium, rows):
    import ctypes as C
    names = (C.c_char_p * max(len(parms), 1))(*[k.encode() for k in parms])
    sizes = np.array([np.atleast_1d(v).size for v in parms.values()] or [0], np.int32)
    values = np.zeros((max(len(parms), 1), 4), F)
    for i, v in enumerate(parms.values()):
        v = np.atleast_1d(np.asarray(v, F))
        values[i, :v.size] = v
    out = np.zeros((rows.shape[0], 34), F)
    rc = lib.ref_material_components(typ.encode(), len(parms), names, _p(sizes), _p(values),
                                     _p(np.array(medium, F)), rows.shape[0], _p(rows), _p(out))
    assert rc == 0, rc
    return out


def oracle_material(typ, parms, medium, rows):
    import oracle
    return oracle.material_components(material_blob(typ, parms), medium, rows)


def material_stem(name):
    """The fixture file of a material case: one per material class."""
    return "mat_" + MATERIALS[name][0].lower()


def material_digest(typ, parms, medium, rows):
    return digest(np.frombuffer(material_blob(typ, parms), np.uint8), np.array(medium, F), rows)
