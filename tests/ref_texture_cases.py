"""Inputs and the independent restatement of the texture pin (tests/test_ref_textures.py).

* images from a fixed-seed generator, in the three formats the device stores (RGB8, RGBA8,
  RGB_FLOAT32), and the lookup rows: edge coordinates first, then uniform ones;
* `lookup`: Bilinear::get and NearestNeighbor::get (textures/Bilinear.h:23-40,
  textures/nearestneighbor.h:40-47) in numpy float32, one operation per rounding (the build uses
  -ffp-contract=off), written from the two headers and not from the kernels or the oracle;
* a scene description (images, textures, materials) that is turned into device objects through
  the rt* API on one side and into a frame blob for the oracle on the other.
"""
import struct

import numpy as np

F = np.float32
ROWS = 1024
ONE_M = np.nextafter(F(1), F(0))
ONE_OVER_255 = F(1) / F(255)          # common/sys/constants.h: one_over_255 = 1.f / 255.f
FORMATS = ("RGB8", "RGBA8", "RGB_FLOAT32")
SIZES = [(2, 2), (3, 5), (5, 3), (8, 8), (7, 2)]       # W x H
THIN_SIZES = [(1, 1), (1, 4), (4, 1)]                  # 1 texel wide or high: the clamped + 1 fetch
COMBOS = [("bilinear", False), ("nearest", False), ("bilinear", True), ("nearest", True)]
IMG_FORMAT_ID = {"RGBA8": 0, "RGB_FLOAT32": 1, "RGB8": 2}   # common/yrt_gpu_types.h ImageFormat


# ---------------------------------------------------------------- images
def image(w, h, fmt, seed):
    """(h, w, channels) texels of a w x h image, row y, column x: uint8 over the full byte range
    with 0 and 255 in texel (0, 0), or float32 in [-0.5, 2). No two channels alike, and no image
    equal to its transpose (checked by test_images_are_asymmetric)."""
    rng = np.random.default_rng(seed)
    if fmt == "RGB_FLOAT32":
        return (F(-0.5) + F(2.5) * rng.random((h, w, 3), dtype=F)).astype(F)
    c = 4 if fmt == "RGBA8" else 3
    a = rng.integers(0, 256, (h, w, c)).astype(np.uint8)
    a[0, 0, 0], a[0, 0, 1] = 0, 255
    if a[0, 0, 2] in (0, 255):
        a[0, 0, 2] = 77
    if c == 4 and w * h > 1:  # alpha 255 in the last texel, 0 in the first row's last, values between elsewhere
        a[-1, -1, 3] = 255
        a[0, -1 if h > 1 else 0, 3] = 0
    elif c == 4:
        a[0, 0, 3] = 128
    return a


def pool_bytes(img, fmt):
    """The 4-channel texels the device and the frame blob store (device/image_io.cpp
    image_from_memory): RGB8 gets alpha 255 (read as exactly 1), RGB_FLOAT32 alpha 1."""
    h, w = img.shape[:2]
    if fmt == "RGB_FLOAT32":
        return np.concatenate([img.astype(F), np.ones((h, w, 1), F)], 2).tobytes()
    if fmt == "RGB8":
        return np.concatenate([img, np.full((h, w, 1), 255, np.uint8)], 2).tobytes()
    return np.ascontiguousarray(img).tobytes()


def texels_rgba(img, fmt):
    """Image::get of every texel as Color4, float32 (h, w, 4): Image3c / Image4c scale a byte by
    one_over_255, an RGB image's alpha is 1."""
    h, w = img.shape[:2]
    if fmt == "RGB_FLOAT32":
        return np.concatenate([img.astype(F), np.ones((h, w, 1), F)], 2)
    c = img.astype(F) * ONE_OVER_255
    if fmt == "RGB8":
        c = np.concatenate([c, np.ones((h, w, 1), F)], 2)
    return c.astype(F)


# ---------------------------------------------------------------- the restatement
def lookup(img, fmt, filt, invert, s, t):
    """Texture::get at (s, t), float32 (n, 4). Bilinear: the x + 1 and y + 1 fetches are clamped to
    W - 1 and H - 1 (the renderer's defined departure; x <= W - 2 unless W == 1, so the clamp
    changes no value of an image at least 2 texels wide and high)."""
    tex = texels_rgba(img, fmt)
    h, w = tex.shape[:2]
    s, t = np.asarray(s, F), np.asarray(t, F)
    s1, t1 = (s - np.floor(s)).astype(F), (t - np.floor(t)).astype(F)
    if filt == "bilinear":
        u = (s1 * F(w)).astype(F) - F(.5)
        v = (t1 * F(h)).astype(F) - F(.5)
        x = np.maximum(0, np.minimum(np.floor(u).astype(np.int32), w - 2))   # clamp(int(floorf(u)), 0, W - 2)
        y = np.maximum(0, np.minimum(np.floor(v).astype(np.int32), h - 2))
        x1, y1 = np.minimum(x + 1, w - 1), np.minimum(y + 1, h - 1)
        ur, vr = (u - x.astype(F)).astype(F), (v - y.astype(F)).astype(F)
        uo, vo = (F(1) - ur).astype(F), (F(1) - vr).astype(F)
        ur, vr, uo, vo = (a[:, None] for a in (ur, vr, uo, vo))
        top = (tex[y, x] * uo).astype(F) + (tex[y, x1] * ur).astype(F)
        bot = (tex[y1, x] * uo).astype(F) + (tex[y1, x1] * ur).astype(F)
        c = (top.astype(F) * vo).astype(F) + (bot.astype(F) * vr).astype(F)
    else:
        si, ti = (s1 * F(w)).astype(F).astype(np.int32), (t1 * F(h)).astype(F).astype(np.int32)
        c = tex[np.clip(ti, 0, h - 1), np.clip(si, 0, w - 1)]
    c = c.astype(F)
    return (F(1) - c).astype(F) if invert else c


# ---------------------------------------------------------------- rows
def edge_values(n):
    """The edge coordinates along an axis of n texels."""
    v = [F(0), F(1), F(-1), F(0.5) / F(n)]
    for k in range(n + 1):
        x = F(k) / F(n)
        v += [np.nextafter(x, F(-9)), x, np.nextafter(x, F(9))]
    v += [(F(n) - F(0.5)) / F(n), ONE_M, F(-1e-9), F(3.25), F(-2.75), F(2 ** 24 + 1)]
    return np.array(v, F)


def st_rows(w, h, seed=0):
    """(ROWS, 2) float32 (s, t): the first dozen edge values of each axis crossed pairwise, then
    every edge value of s beside one of t, then uniform in [-2, 3)."""
    es, et = edge_values(w), edge_values(h)
    rows = [(a, b) for a in es[:12] for b in et[:12]]
    rows += [(es[i % len(es)], et[i % len(et)]) for i in range(max(len(es), len(et)))]
    rows += [(es[i % len(es)], et[(i + 5) % len(et)]) for i in range(max(len(es), len(et)))]
    e = np.array(rows, F)
    assert len(e) < ROWS // 2
    rng = np.random.default_rng(4000 + 64 * w + h + seed)
    st = (F(-2) + F(5) * rng.random((ROWS, 2), dtype=F)).astype(F)
    st[:len(e)] = e
    return st


# ---------------------------------------------------------------- scene descriptions
class Case:
    """images: name -> (fmt, texels); textures: name -> (filter, invert, image name); materials:
    [(class, {parameter: float | 2 floats | 3 floats}, {parameter: texture name})], one triangle
    each, in slot order. Images enter the device's texel pool in the order the materials name them
    (a material's texture parameters in the order of its GpuMaterial::tex slots)."""

    TEX_SLOTS = ("map_d", "map_Kd", "map_Ks", "map_Ns", "map_Bump", "Kd")

    def __init__(self, images, textures, materials):
        self.images, self.textures, self.materials = images, textures, materials

    # -- the device side
    def build(self, dev):
        """Commits the case on `dev`; returns (scene, [primitive per material])."""
        img, tex = {}, {}
        for name, (fmt, a) in self.images.items():
            data = a if fmt != "RGB_FLOAT32" else a.astype(F)
            img[name] = dev.rtNewImage(fmt, a.shape[1], a.shape[0], np.ascontiguousarray(data))
        for name, (filt, invert, image_name) in self.textures.items():
            tex[name] = dev.rtNewTexture(filt)
            dev.rtSetImage(tex[name], "image", img[image_name])
            if invert:
                dev.rtSetBool1(tex[name], "invert", True)
            dev.rtCommit(tex[name])
        scene = dev.rtNewScene("default")
        prims = []
        for slot, (cls, floats, texs) in enumerate(self.materials):
            m = dev.rtNewMaterial(cls)
            for k, v in floats.items():
                v = np.atleast_1d(np.asarray(v, F))
                {1: dev.rtSetFloat1, 2: dev.rtSetFloat2, 3: dev.rtSetFloat3}[v.size](m, k, *[float(x) for x in v])
            for k in sorted(texs, key=self.TEX_SLOTS.index):
                dev.rtSetTexture(m, k, tex[texs[k]])
            dev.rtCommit(m)
            mesh = dev.rtNewShape("trianglemesh")
            pos = np.array([[3 * slot, 0, 0], [3 * slot + 1, 0, 0], [3 * slot, 1, 0]], F)
            for name, a, typ, step in (("positions", pos, "float3", 12), ("indices", np.array([[0, 1, 2]], np.int32), "int3", 12)):
                dev.rtSetArray(mesh, name, typ, dev.rtNewData("immutable", a), len(a), step)
            dev.rtCommit(mesh)
            prims.append(dev.rtNewShapePrimitive(mesh, m))
            dev.rtSetPrimitive(scene, slot, prims[-1])
        dev.rtCommit(scene)
        return scene, prims

    # -- the oracle side: a frame blob (device/export.cpp's format) of the images, the textures and
    # ONE material (oracle.material_components shades the blob's first material)
    def blob(self, material=0):
        def s(x):
            b = x.encode()
            return struct.pack("<I", len(b)) + b

        ids, objs = {}, []
        for name, (fmt, a) in self.images.items():
            data = pool_bytes(a, fmt)
            ids["i" + name] = len(objs)
            objs.append(struct.pack("<I", 2) + s("image") + struct.pack("<I", 0) +
                        struct.pack("<iiiI", a.shape[1], a.shape[0], IMG_FORMAT_ID[fmt], len(data)) + data)
        for name, (filt, invert, image_name) in self.textures.items():
            ids["t" + name] = len(objs)
            objs.append(struct.pack("<I", 3) + s(filt) + struct.pack("<I", 2) +
                        s("image") + struct.pack("<Ii", 14, ids["i" + image_name]) +
                        s("invert") + struct.pack("<I4i", 1, int(invert), 0, 0, 0))
        if self.materials:
            cls, floats, texs = self.materials[material]
            o = struct.pack("<I", 4) + s(cls) + struct.pack("<I", len(floats) + len(texs))
            for k, v in floats.items():
                v = np.atleast_1d(np.asarray(v, F))
                o += s(k) + struct.pack("<I", {1: 9, 2: 10, 3: 11}[v.size])
                o += np.concatenate([v, np.zeros(4 - v.size, F)]).astype("<f4").tobytes()
            for k, name in texs.items():
                o += s(k) + struct.pack("<Ii", 15, ids["t" + name])
            objs.append(o)
        return b"YRTF" + struct.pack("<II", 1, len(objs)) + b"".join(objs) + struct.pack("<IiiI", 0, -1, -1, 0)

    def texture_index(self, name):
        return list(self.textures).index(name)


def neighbours(fmt, seed):
    """Two small images of the test image's pool part (the 8-bit images and the float images are
    pooled apart) and one of the other part: what lies before and after the image under test."""
    if fmt == "RGB_FLOAT32":
        return {"A": ("RGB_FLOAT32", image(3, 2, "RGB_FLOAT32", seed + 1)), "C": ("RGB_FLOAT32", image(2, 3, "RGB_FLOAT32", seed + 2)),
                "D": ("RGBA8", image(3, 3, "RGBA8", seed + 3))}
    return {"A": ("RGBA8", image(3, 2, "RGBA8", seed + 1)), "C": ("RGB8", image(2, 3, "RGB8", seed + 2)),
            "D": ("RGB_FLOAT32", image(2, 2, "RGB_FLOAT32", seed + 3))}


def lookup_case(w, h, fmt, last=False, follower=None):
    """The scene of one image under test, T: four Obj materials whose map_d (texture slot 0, the
    descriptor copy in the geometry record) is T through each of COMBOS and whose map_Ks is T
    through the next combination, with neighbour images so that T is the second image of its pool
    part (last: the last one). follower: another image in place of the one that follows T."""
    seed = 1000 * w + 10 * h + FORMATS.index(fmt)
    nb = neighbours(fmt, seed)
    if follower is not None:
        nb["C"] = follower
    images = {"A": nb["A"], "T": (fmt, image(w, h, fmt, seed)), "C": nb["C"], "D": nb["D"]}
    textures = {f"T{j}": (filt, inv, "T") for j, (filt, inv) in enumerate(COMBOS)}
    textures.update(A=("nearest", False, "A"), C=("bilinear", False, "C"), D=("nearest", True, "D"))
    first = ("MatteTextured", {}, {"Kd": "A"})
    objs = [("Obj", {"d": 1.0}, {"map_d": f"T{j}", "map_Kd": "C", "map_Ks": f"T{(j + 1) % 4}", "map_Ns": "D"}) for j in range(4)]
    if last:  # A, C, then T
        first = ("Obj", {}, {"map_d": "A", "map_Kd": "C"})
        objs = [("Obj", {"d": 1.0}, {"map_d": f"T{j}", "map_Ks": f"T{(j + 1) % 4}", "map_Ns": "D"}) for j in range(4)]
    return Case(images, textures, [first] + objs)
