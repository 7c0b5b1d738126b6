"""numpy helpers of tests/test_denoise_albedo.py (the texture-preserving filter): the
texture lookups a material performs (textures/Bilinear.h, textures/nearestneighbor.h), the
modulation, the demodulated filter on top of denoise_ref.atrous, and scenes whose meshes carry
their own materials and texture coordinates. Written from the definitions, not from the kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np

import denoise_ref as ref

F = np.float32
QUAD_IDX = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
QUAD_ST = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)   # texture coordinates of a quad's four vertices


# ----------------------------------------------------------------------------- framebuffers
def stride(fmt, w):
    return {"RGB8": (3 * w + 3) // 4 * 4, "RGBA8": 4 * w, "RGB_FLOAT32": 12 * w, "RGBA_FLOAT32": 16 * w}[fmt]


def mapped(d, fb, fmt, w, h, write=None):
    """The mapped framebuffer's bytes, row padding included, as (h, stride) uint8 (a copy); write:
    bytes of the same shape stored into the mapped pixels first."""
    p = d.rtMapFrameBuffer(fb)
    a = np.ctypeslib.as_array((C.c_uint8 * (stride(fmt, w) * h)).from_address(p)).reshape(h, stride(fmt, w))
    if write is not None:
        a[...] = write
    a = a.copy()
    d.rtUnmapFrameBuffer(fb)
    return a


def pixels(raw, fmt, w):
    """(h, w, channels) view of `mapped` bytes: uint8 or float32."""
    h = raw.shape[0]
    if fmt == "RGB8":
        return raw[:, :3 * w].reshape(h, w, 3)
    if fmt == "RGBA8":
        return raw.reshape(h, w, 4)
    return raw.view(F).reshape(h, w, 3 if fmt == "RGB_FLOAT32" else 4)


def reldev(got, want):
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1 / 255)).max())


# ----------------------------------------------------------------------------- textures
def texture_image(n):
    """(n, n, 3) float32, row y, column x: texel (x, y) channel k = (64 + k + 3 (x + n y)) / 256:
    distinct dyadic values in [1/4, 1) for n <= 8, neighbours 3/256 apart along x and 3 n / 256 along
    y, so a transposed or shifted lookup shows."""
    y, x, k = np.mgrid[0:n, 0:n, 0:3]
    return ((64 + k + 3 * (x + n * y)) / 256.0).astype(F)


def lookup_nearest(img, s, t):
    """nearestneighbor.h in float32, as the material does it: texel (int(s1 W), int(t1 H)) clamped
    into the image, s1 = s - floor(s). img (H, W, c); s, t arrays -> (..., c) float32."""
    h, w = img.shape[:2]
    s, t = np.asarray(s, F), np.asarray(t, F)
    s1, t1 = s - np.floor(s), t - np.floor(t)
    ix = np.clip((s1 * F(w)).astype(np.int32), 0, w - 1)
    iy = np.clip((t1 * F(h)).astype(np.int32), 0, h - 1)
    return img[iy, ix]


def texel_boundary_distance(s, t, w, h):
    """Distance, in units of (s, t), of each point from the nearest texel boundary of a w x h image."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    return np.minimum(np.abs(s * w - np.round(s * w)) / w, np.abs(t * h - np.round(t * h)) / h)


def lookup_bilinear(img, s, t):
    """Bilinear.h in float64: u = s1 W - 1/2, x = clamp(floor(u), 0, W - 2), ratio u - x (outside
    [0, 1] in the half texel along the border: the lookup extrapolates there), and the same in t."""
    h, w = img.shape[:2]
    img = img.astype(np.float64)
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    u = (s - np.floor(s)) * w - 0.5
    v = (t - np.floor(t)) * h - 0.5
    x = np.clip(np.floor(u).astype(np.int64), 0, w - 2)
    y = np.clip(np.floor(v).astype(np.int64), 0, h - 2)
    ur, vr = (u - x)[..., None], (v - y)[..., None]
    return (img[y, x] * (1 - ur) + img[y, x + 1] * ur) * (1 - vr) + (img[y + 1, x] * (1 - ur) + img[y + 1, x + 1] * ur) * vr


# ----------------------------------------------------------------------------- the filter
def modulation(albedo4, power, floor, dtype=np.float64):
    """m = max(albedo, floor) ^ power per channel on hit pixels (albedo4.w != 0), 1 on a miss; power
    and floor are the float32 values the library receives. (H, W, 3) of `dtype`."""
    a = np.asarray(albedo4)
    hit = a[..., 3] != 0
    m = np.power(np.maximum(a[..., :3].astype(dtype), dtype(F(floor))), dtype(F(power))).astype(dtype)
    m[~hit] = 1
    return m


def demodulated_atrous(c0, pos4, nrm4, albedo4, iterations, power, floor, **weights):
    """denoise_ref.atrous on c0 / m, times m, in float64: the colour weight acts on the quotient."""
    m = modulation(albedo4, power, floor)
    return ref.atrous(np.asarray(c0, np.float64) / m, pos4, nrm4, iterations, **weights) * m


# ----------------------------------------------------------------------------- scenes
def textured_quads():
    """Two quads for a camera at the origin looking along +z, with dyadic corners and the unit
    square as texture coordinates: `near` at z = 2, (s, t) = (x + 1, y + 1/2); `tilt` turned 45
    degrees about y, x + z = 5, (s, t) = (x / 2, (y + 1) / 2)."""
    near = np.array([[-1, -0.5, 2], [0, -0.5, 2], [0, 0.5, 2], [-1, 0.5, 2]], F)
    tilt = np.array([[0, -1, 5], [2, -1, 3], [2, 1, 3], [0, 1, 5]], F)
    return near, tilt


def quad_st(pos4, near):
    """(s, t) of textured_quads' hit points, float64 (the parametrisation above is exact in it)."""
    p = np.asarray(pos4, np.float64)
    if near:
        return p[..., 0] + 1.0, p[..., 1] + 0.5
    return p[..., 0] / 2.0, (p[..., 1] + 1.0) / 2.0


def texture(dev, kind, image, fmt="RGB_FLOAT32"):
    im = dev.rtNewImage(fmt, image.shape[1], image.shape[0], image)
    tx = dev.rtNewTexture(kind)
    dev.rtSetImage(tx, "image", im)
    dev.rtCommit(tx)
    return tx


def material(dev, kind, floats=(), textures=()):
    m = dev.rtNewMaterial(kind)
    for name, v in floats:
        if np.ndim(v) == 0:
            dev.rtSetFloat1(m, name, float(v))
        else:
            dev.rtSetFloat3(m, name, *[float(x) for x in v])
    for name, tx in textures:
        dev.rtSetTexture(m, name, tx)
    dev.rtCommit(m)
    return m


class MaterialScene:
    """A committed scene of quads, [(corners (4, 3), material handle)], each with QUAD_ST as its
    texture coordinates, in primitive slots 0.., and denoise_ref's pinhole camera at the origin
    looking along +z (60 degrees). `dev` and `scene` as trace_scenes.MeshScene has them, so
    denoise_ref.add_triangle_light serves (slot 2: two quads)."""

    def __init__(self, dev, quads):
        from test_cpu_host import yrt_lookat
        d = self.dev = dev
        self.scene = d.rtNewScene("default")
        for slot, (corners, mat) in enumerate(quads):
            mesh = d.rtNewShape("trianglemesh")
            arrays = (("positions", np.ascontiguousarray(corners, F), "float3", 12),
                      ("texcoords", QUAD_ST, "float2", 8), ("indices", QUAD_IDX, "int3", 12))
            for name, a, typ, step in arrays:
                d.rtSetArray(mesh, name, typ, d.rtNewData("immutable", a), len(a), step)
            d.rtCommit(mesh)
            d.rtSetPrimitive(self.scene, slot, d.rtNewShapePrimitive(mesh, mat))
        d.rtCommit(self.scene)
        self.camera = d.rtNewCamera("pinhole")
        d.rtSetTransform(self.camera, "local2world", yrt_lookat((0, 0, 0), (0, 0, 1), (0, 1, 0)))
        d.rtSetFloat1(self.camera, "angle", 60.0)
        d.rtSetFloat1(self.camera, "aspectRatio", 1.0)
        d.rtCommit(self.camera)


# ----------------------------------------------------------------------------- a textured room
ROOM = (556.0, 548.8, 559.2)   # the Cornell box's interior


def room_textures():
    """Two 10 x 10 RGB textures: 8 x 8 saturated random colours (48..249 of 255, fixed seeds) with the
    border texels repeated once, since Bilinear.h extrapolates in the half texel along an image's
    border and would leave [0, 1] there. Through the loader's bilinear filter a texel spans several
    pixels of a 64 x 64 frame."""
    return [np.pad(np.random.default_rng(seed).integers(48, 250, (8, 8, 3)).astype(np.uint8), ((1, 1), (1, 1), (0, 0)),
                   mode="edge") for seed in (31, 32)]


def room_quads():
    """[(corners (4, 3), texture index)]: the five walls of the Cornell box (open towards the
    camera) with texture 0 and the top and sides of a block standing in it with texture 1; every quad
    carries QUAD_ST."""
    X, Y, Z = ROOM
    q = [([(0, 0, 0), (X, 0, 0), (X, 0, Z), (0, 0, Z)], 0), ([(0, Y, 0), (X, Y, 0), (X, Y, Z), (0, Y, Z)], 0),
         ([(0, 0, Z), (X, 0, Z), (X, Y, Z), (0, Y, Z)], 0), ([(X, 0, 0), (X, 0, Z), (X, Y, Z), (X, Y, 0)], 0),
         ([(0, 0, 0), (0, 0, Z), (0, Y, Z), (0, Y, 0)], 0)]
    x0, x1, y1, z0, z1 = 170.0, 390.0, 210.0, 180.0, 400.0
    q += [([(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)], 1), ([(x0, 0, z0), (x1, 0, z0), (x1, y1, z0), (x0, y1, z0)], 1),
          ([(x0, 0, z1), (x1, 0, z1), (x1, y1, z1), (x0, y1, z1)], 1), ([(x0, 0, z0), (x0, 0, z1), (x0, y1, z1), (x0, y1, z0)], 1),
          ([(x1, 0, z0), (x1, 0, z1), (x1, y1, z1), (x1, y1, z0)], 1)]
    return [(np.array(c, F), t) for c, t in q]


def write_room(directory):
    """Writes room.xml (MatteTextured quads under the Cornell box's quad light) and its two .ppm
    textures into `directory`; returns the XML's path."""
    from pathlib import Path
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    for k, img in enumerate(room_textures()):
        (directory / f"room_tex{k}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    fmt = lambda a: " ".join("%.9g" % v for v in np.asarray(a).reshape(-1))  # noqa: E731
    out = ['<?xml version="1.0"?>', "<scene>", "  <Group>"]
    for corners, tex in room_quads():
        out += ["    <TriangleMesh>", "      <positions>" + fmt(corners) + "</positions>",
                "      <texcoords>" + fmt(QUAD_ST) + "</texcoords>", "      <triangles>" + fmt(QUAD_IDX) + "</triangles>",
                '      <material>\n        <code>"MatteTextured"</code>\n        <parameters>',
                f'          <texture name="Kd">"room_tex{tex}.ppm"</texture>',
                "        </parameters>\n      </material>", "    </TriangleMesh>"]
    out += ["    <QuadLight>", "      <AffineSpace>130 0 0 213.0  0 0 1 548.77  0 105 0 227.0</AffineSpace>",
            "      <L>30 30 27</L>", "    </QuadLight>", "  </Group>", "</scene>", ""]
    path = directory / "room.xml"
    path.write_text("\n".join(out))
    return path


def room_args(xml, size, spp):
    """The room through the Cornell box's camera, depth 5, gamma 2.2, RGB_FLOAT32."""
    return ["-i", str(xml), "-vp", "278", "273", "-800", "-vi", "278", "273", "0", "-vu", "0", "1", "0", "-fov", "37",
            "-depth", "5", "-renderer", "pathtracer", "-size", str(size), str(size),
            "-spp", str(spp), "-fb", "RGB_FLOAT32", "-gamma", "2.2"]
