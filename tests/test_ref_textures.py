"""The device's Material::shade and its texture lookup, probed bit for bit.

The probe (yrtDebugMaterial: k_check_material / k_check_textures, kernels/k_checks.h) reads one
primitive's record from a committed scene's uploaded tables with geom_burst, as k_shade does, and
calls shade_material, comp_eval, comp_sample and tex_get / tex_get_rec as they stand.

  a  the device's shade_material of the nine texture-free materials, built through rtNewMaterial /
     rtSet* / rtCommit, == the reference's own answers (tests/golden/ref_shade_mat_*.npz), through
     the every-material instantiation and every specialized one that holds the material;
  b  the texture lookup, three witnesses: a numpy float32 restatement of Bilinear.h and
     nearestneighbor.h (tests/ref_texture_cases.py) == the oracle; the host-built 2x2 footprint
     records == the row-major pool; on the GPU the probe == numpy, and texture slot 0 through the
     texture table == slot 0 through the descriptor copy in the geometry record;
  c  the textured materials (MatteTextured, Uber, ThinDielectric, Obj): device == oracle through
     every instantiation that holds them, and on the CPU the oracle's textured classes over a
     constant image == its reference-pinned untextured ones.

No comparison uses a tolerance; the rules are tests/test_ref_shade.py's (bits; a NaN equals a NaN;
an exactly zero colour may differ in the sign of the zero; the direction of a rejected sample is
not compared, and rejected rows are at most a quarter of the rows a component is compared on).
There is no reference value for a bilinear image 1 texel wide or high (the reference reads outside
it): there the expected value is the restatement with the + 1 fetches clamped into the image.
"""
import functools

import numpy as np
import pytest

import oracle
import ref_shade_cases as R
import ref_texture_cases as T
import test_ref_shade as S

F = np.float32
IMAGES = [(w, h, fmt) for (w, h) in T.SIZES + T.THIN_SIZES for fmt in T.FORMATS]
image_ids = [f"{w}x{h}-{fmt}" for w, h, fmt in IMAGES]
# the shade kernel's specialized material sets (kernels/pathtrace.hip kShadeVariants) by material class
SETS_OF = {"Matte": ["spheres", "collada"], "MetallicPaint": ["spheres", "stereo"], "ThinDielectric": ["collada"],
           "Uber": ["uber", "stereo", "collada"], "MatteTextured": ["stereo"], "Obj": ["obj"]}


def _sets(cls, name=""):
    glitter = cls == "MetallicPaint" and "glitter" in name   # MAT_METALLIC_GLITTER: in no specialized set
    return ["all"] + ([] if glitter else SETS_OF.get(cls, []))


# ---------------------------------------------------------------- b: the generators
def test_images_are_asymmetric():
    """No image equals its transpose or has two equal channels, and the 8-bit ones hold 0 and 255:
    a transposed lookup or a swapped channel cannot go unseen."""
    for w, h, fmt in IMAGES:
        a = T.image(w, h, fmt, 1000 * w + 10 * h + T.FORMATS.index(fmt))
        assert a.shape[:2] == (h, w) and w * h <= 64
        for i in range(a.shape[2]):
            for j in range(i + 1, a.shape[2]):
                assert not np.array_equal(a[..., i], a[..., j]), (w, h, fmt, i, j)
        if w == h and w > 1:
            assert not np.array_equal(a, a.transpose(1, 0, 2))
        if fmt != "RGB_FLOAT32":
            assert a.dtype == np.uint8 and a.min() == 0 and a.max() == 255
        else:
            assert np.isfinite(a).all()


@pytest.mark.parametrize("w,h", T.SIZES + T.THIN_SIZES)
def test_rows_cover_the_edges(w, h):
    st = T.st_rows(w, h)
    assert st.shape == (T.ROWS, 2) and st.dtype == F and np.isfinite(st).all()
    for axis, n in ((0, w), (1, h)):
        have = set(st[:, axis].tolist())
        want = [0.0, 1.0, -1.0, F(0.5) / F(n), (F(n) - F(0.5)) / F(n), T.ONE_M, F(-1e-9), 3.25, -2.75, F(2 ** 24 + 1)]
        for k in range(n + 1):
            x = F(k) / F(n)
            want += [x, np.nextafter(x, F(-9)), np.nextafter(x, F(9))]
        assert {float(F(v)) for v in want} <= have, (axis, n)
    # at -1e-9 the fraction s - floor(s) is exactly 1; at 2^24 + 1 it is lost
    assert F(-1e-9) - np.floor(F(-1e-9)) == F(1) and F(2 ** 24 + 1) - np.floor(F(2 ** 24 + 1)) == 0
    es, et = T.edge_values(w)[:12], T.edge_values(h)[:12]   # the first dozen values of each axis, crossed
    assert {(float(a), float(b)) for a in es for b in et} == {(float(a), float(b)) for a, b in st[:144]}
    assert (st[T.ROWS // 2:] >= -2).all() and (st[T.ROWS // 2:] < 3).all()


def test_restatement_extrapolates_at_the_border():
    """The properties the rows are there for, on the restatement itself: at s = -1e-9 the bilinear
    lookup sits on x = W - 2 with ratio 1.5, and nearest on the last texel."""
    img = T.image(5, 3, "RGB_FLOAT32", 9)
    tex = T.texels_rgba(img, "RGB_FLOAT32")
    s, t = np.array([-1e-9], F), np.array([0.5], F)           # v = 1, y = 1, ratio 0
    got = T.lookup(img, "RGB_FLOAT32", "bilinear", False, s, t)[0]
    want = (tex[1, 3] * F(-0.5) + tex[1, 4] * F(1.5)) * F(1) + (tex[2, 3] * F(-0.5) + tex[2, 4] * F(1.5)) * F(0)
    assert np.array_equal(got, want.astype(F))
    assert np.array_equal(T.lookup(img, "RGB_FLOAT32", "nearest", False, s, t)[0], tex[1, 4])
    assert np.array_equal(T.lookup(img, "RGB_FLOAT32", "nearest", True, s, t)[0], F(1) - tex[1, 4])


# ---------------------------------------------------------------- b: numpy == oracle
@functools.lru_cache(maxsize=None)
def _expected(w, h, fmt):
    """(st, {texture name: RGBA (ROWS, 4)}) of lookup_case(w, h, fmt)'s textures over T, by numpy."""
    st = T.st_rows(w, h)
    img = T.image(w, h, fmt, 1000 * w + 10 * h + T.FORMATS.index(fmt))
    return st, {f"T{j}": T.lookup(img, fmt, filt, inv, st[:, 0], st[:, 1]) for j, (filt, inv) in enumerate(T.COMBOS)}


@pytest.mark.parametrize("w,h,fmt", IMAGES, ids=image_ids)
def test_restatement_equals_the_oracle(w, h, fmt):
    """Bilinear::get and NearestNeighbor::get, invert off and on: the numpy restatement == the
    oracle's tex_get, by bits, on the 1024 rows."""
    case = T.lookup_case(w, h, fmt)
    blob = case.blob()
    st, want = _expected(w, h, fmt)
    for name, rgba in want.items():
        got = oracle.texture_get(blob, case.texture_index(name), st[:, 0], st[:, 1])
        bad = np.where(~R.same_bits(got, rgba))[0]
        assert bad.size == 0, (name, case.textures[name], bad[:8].tolist(), st[bad[:2]].tolist(), got[bad[:2]].tolist(),
                               rgba[bad[:2]].tolist())
    # and the neighbour images through their own textures (other sizes, the other pool part)
    for name in ("A", "C", "D"):
        filt, inv, im = case.textures[name]
        f, a = case.images[im]
        got = oracle.texture_get(blob, case.texture_index(name), st[:, 0], st[:, 1])
        assert R.same_bits(got, T.lookup(a, f, filt, inv, st[:, 0], st[:, 1])).all(), name


# ---------------------------------------------------------------- b: the pools
def _pool_images(case, pools):
    """name -> (width, height, format id, offset) of the case's images: the pool holds the 8-bit
    images in the order the materials name them, then the float ones."""
    recs = pools["images"]
    order = []
    for _, _, texs in case.materials:
        for k in sorted(texs, key=T.Case.TEX_SLOTS.index):
            im = case.textures[texs[k]][2]
            if im not in order:
                order.append(im)
    assert len(order) == len(recs)
    out = {}
    for name, r in zip(order, recs):
        fmt, a = case.images[name]
        assert (r[0], r[1], r[2]) == (a.shape[1], a.shape[0], T.IMG_FORMAT_ID[fmt]), name
        out[name] = (int(r[0]), int(r[1]), int(r[2]), int(r[4]) | (int(r[5]) << 32))
    return out


def _check_pools(case, pools, names):
    """The row-major pool holds each image's texels at its offset, and footprint record (x, y) of an
    8-bit image holds texels (x, y), (x', y), (x, y'), (x', y') of that image, x' = min(x + 1, W - 1),
    for every record a lookup can address (x <= max(W - 2, 0), y <= max(H - 2, 0))."""
    imgs = _pool_images(case, pools)
    texels, quads = pools["texels"], pools["quads"]
    eight = sorted(o for (_, _, f, o) in imgs.values() if f != 1)
    floats = sorted(o for (_, _, f, o) in imgs.values() if f == 1)
    assert not eight or not floats or eight[-1] < floats[0]      # 8-bit images first
    for name in names:
        w, h, f, off = imgs[name]
        fmt, a = case.images[name]
        data = np.frombuffer(T.pool_bytes(a, fmt), np.uint8)
        assert off % 16 == 0 and np.array_equal(texels[off:off + data.size], data), name
        if f == 1:
            continue
        word = data.view(np.uint32).reshape(h, w)
        for y in range(max(h - 1, 1)):
            for x in range(max(w - 1, 1)):
                x1, y1 = min(x + 1, w - 1), min(y + 1, h - 1)
                want = [word[y, x], word[y, x1], word[y1, x], word[y1, x1]]
                assert quads[off // 4 + y * w + x].tolist() == want, (name, x, y)
    return imgs


@pytest.mark.parametrize("fmt", T.FORMATS)
def test_footprint_records_agree_with_the_pool(host_device, fmt):
    """The host-built texQuads of a committed scene against its row-major pool, image under test
    second in its pool part and (once per size) last."""
    for w, h in T.SIZES + T.THIN_SIZES:
        for last in (False, True):
            case = T.lookup_case(w, h, fmt, last=last)
            scene, _ = case.build(host_device)
            pools = host_device.debug_texture_pools(scene)
            imgs = _check_pools(case, pools, ["A", "T", "C", "D"])
            part = sorted(o for (_, _, f, o) in imgs.values() if (f == 1) == (fmt == "RGB_FLOAT32"))
            assert part.index(imgs["T"][3]) == (len(part) - 1 if last else 1)
            host_device.rtDecRef(scene)


@pytest.mark.parametrize("w,h", T.THIN_SIZES)
def test_thin_image_does_not_depend_on_its_follower(host_device, w, h):
    """An image 1 texel wide or high: its footprint records hold its own texels only, whatever
    image follows it in the pool, and so does the oracle's lookup."""
    st, want = _expected(w, h, "RGBA8")
    seen = []
    for follower in (("RGB8", T.image(2, 3, "RGB8", 71)), ("RGBA8", np.full((3, 3, 4), 255, np.uint8))):
        case = T.lookup_case(w, h, "RGBA8", follower=follower)
        scene, _ = case.build(host_device)
        pools = host_device.debug_texture_pools(scene)
        _, _, _, off = _check_pools(case, pools, ["T"])["T"]
        seen.append(pools["quads"][off // 4:off // 4 + w * h].copy())
        host_device.rtDecRef(scene)
        for name, rgba in want.items():
            got = oracle.texture_get(case.blob(), case.texture_index(name), st[:, 0], st[:, 1])
            assert R.same_bits(got, rgba).all(), name
    assert np.array_equal(seen[0], seen[1])


# ---------------------------------------------------------------- c: the textured cases
def _uber_image():
    a = T.image(8, 8, "RGBA8", 5001)
    a[2:4, 2:4, 3] = 255       # a 2 x 2 block of alpha 255 (no transmission component) and one more texel of 0
    a[5, 5, 3] = 0
    return a


def _bump_image():
    """Blue 200..255 and red, green about the middle: b = 2 c - 1 keeps the bumped normal within
    about 25 degrees of Ns, so that most rows still see the surface from above."""
    a = T.image(5, 3, "RGB8", 5002)
    a[..., 2] = 200 + a[..., 2] % 56
    a[..., :2] = 96 + a[..., :2] % 64
    return a


_MAPS = {"map_d": ("bilinear", "RGB8", 3, 5), "map_Kd": ("nearest", "RGBA8", 5, 3), "map_Ks": ("bilinear", "RGB_FLOAT32", 2, 2),
         "map_Ns": ("nearest", "RGB8", 7, 2), "map_Bump": ("bilinear", "RGB8", 5, 3)}


def _obj_case(maps, floats):
    images, textures = {}, {}
    for j, (k, (filt, fmt, w, h)) in enumerate(_MAPS.items()):
        if k in maps:
            images[k] = (fmt, _bump_image() if k == "map_Bump" else T.image(w, h, fmt, 5100 + j))
            textures[k] = (filt, False, k)
    first = next(k for k in _MAPS if k in maps)
    w, h = images[first][1].shape[1], images[first][1].shape[0]
    return T.Case(images, textures, [("Obj", floats, {k: k for k in maps})]), (w, h), "plastic_scene"


def _kd_case(cls, fmt, img, filt, invert, floats, rows_of):
    case = T.Case({"K": (fmt, img)}, {"K": (filt, invert, "K")}, [(cls, floats, {"Kd": "K"})])
    return case, (img.shape[1], img.shape[0]), rows_of


_OBJ = {"d": 0.75, "Kd": (0.8, 0.6, 0.4), "Ks": (0.5, 0.7, 0.9), "Ns": 40.0}


@functools.lru_cache(maxsize=None)
def _textured_cases():
    """name -> (Case, (W, H) of the image the (s, t) rows are made for, the MATERIALS name whose
    material_rows supply the directions)"""
    uber = {"s0": (0.25, -0.5), "ds": (1.5, 0.75), "eta": 1.45}
    c = {
        "matte_textured": _kd_case("MatteTextured", "RGB8", T.image(5, 3, "RGB8", 5003), "bilinear", False,
                                   {"s0": (0.25, -0.5), "ds": (1.5, 0.75)}, "matte_scene"),
        # Uber's three specular branches (Uber.h): reflectivity > 0; roughness == 0; a microfacet lobe
        "uber_reflective": _kd_case("Uber", "RGBA8", _uber_image(), "bilinear", False, dict(uber, reflectivity=0.5),
                                    "plastic_scene"),
        "uber_smooth": _kd_case("Uber", "RGBA8", _uber_image(), "nearest", False, dict(uber, roughness=0.0),
                                "plastic_scene"),
        "uber_rough": _kd_case("Uber", "RGBA8", _uber_image(), "nearest", False, {"eta": 1.45, "roughness": 0.05},
                               "plastic_scene"),
        # an inverted RGB8 image: alpha 1 - 1 = 0, so the Lambertian is zero and the opacity 1
        # (nearest: a bilinear blend of four alphas of 1 is 1 only up to an ulp)
        "uber_inverted_rgb8": _kd_case("Uber", "RGB8", T.image(3, 5, "RGB8", 5004), "nearest", True,
                                       dict(uber, reflectivity=0.5), "plastic_scene"),
        "thindielectric_textured": _kd_case("ThinDielectric", "RGB8", T.image(7, 2, "RGB8", 5005), "bilinear", False,
                                            {"s0": (0.5, 0.125), "ds": (0.75, 2.0), "eta": 1.5, "thickness": 0.4,
                                             "transparency": 0.8}, "thindielectric"),
        "obj_all": _obj_case(list(_MAPS), _OBJ),
        # Kd == 0 drops the Lambertian and d == 1 the transmission: the specular lobe alone
        "obj_specular_only": _obj_case(["map_Ks"], {"d": 1.0, "Kd": (0.0, 0.0, 0.0), "Ks": (0.5, 0.7, 0.9), "Ns": 40.0}),
    }
    for k in _MAPS:
        c["obj_" + k] = _obj_case([k], _OBJ)
    return c


def _textured_rows(name):
    case, (w, h), rows_of = _textured_cases()[name]
    return np.concatenate([R.material_rows(rows_of), T.st_rows(w, h, seed=1)], 1)


@functools.lru_cache(maxsize=None)
def _textured_oracle(name):
    case = _textured_cases()[name][0]
    out = oracle.material_components(case.blob(), R.VACUUM, _textured_rows(name))
    out.setflags(write=False)
    return out


def _check_textured(label, got, want, strict=False):
    """_check_material's rules where the component count varies from row to row (a texel decides
    it): counts by bits; slot k on the rows that have a component k, the rest of the slot by bits
    (zero). strict: no row's direction is exempt, and so no cap applies (a case whose component is
    zero on every row by construction: every sample of it is a rejected one)."""
    assert np.array_equal(got[:, 0].view(np.int32), want[:, 0].view(np.int32)), label + ": component counts"
    count = want[:, 0].view(np.int32)
    assert count.min() >= 0 and count.max() <= 3
    for k in range(3):
        c = slice(1 + 11 * k, 12 + 11 * k)
        have = count > k
        assert np.array_equal(got[~have, c].view(np.uint32), want[~have, c].view(np.uint32)), (label, k)
        if not have.any():
            continue
        g, w = got[have, c], want[have, c]
        rej = None if strict else R.rejected(w[:, 4:7], w[:, 10])
        S._check(f"{label} component {k}", g, w, slice(1, 7), slice(7, 10), rej)


STRICT = {"uber_inverted_rgb8"}   # Lambertian and reflection are zero on every row: nothing is exempted


@pytest.mark.parametrize("name", list(_textured_cases()))
def test_textured_cases_meet_the_rejected_cap(name):
    """The oracle alone: every component slot of every textured case is compared with its direction
    on at least three quarters of the rows that have it (the condition _check asserts), the counts
    vary where the case says they do, and the strict case's exempt-nothing rule is well founded:
    its components set a direction on every row."""
    out = _textured_oracle(name)
    _check_textured(f"textured {name} oracle/oracle", out.copy(), out, strict=name in STRICT)
    count = out[:, 0].view(np.int32)
    if name.startswith("uber_") and name not in STRICT:
        assert {2, 3} <= set(count.tolist())          # alpha 255: no transmission component
    if name in STRICT:
        assert (count == 3).all() and (out[:, 2:8] == 0).all()    # the Lambertian: zero colours on every row
        assert np.isfinite(out[:, 8:11]).all() and (np.abs(out[:, 8:11]).sum(1) > 0).all()
    if name == "obj_specular_only":
        assert (count == 1).all() and (out[:, 1].view(np.uint32) == 0x10).all()
    if name == "obj_map_d":
        assert {2, 3} <= set(count.tolist())


def _constant_case(cls, colour8, floats):
    img = np.broadcast_to(np.array(colour8, np.uint8), (3, 2, 3)).copy()
    return T.Case({"K": ("RGB8", img)}, {"K": ("nearest", False, "K")}, [(cls, floats, {"Kd": "K"})])


def test_textured_classes_reduce_to_the_pinned_ones():
    """The tie to the reference-pinned classes: over a constant image of colour c through a
    nearest-neighbour texture, the oracle's MatteTextured == its Matte with reflectance c, and its
    textured ThinDielectric == the untextured one with transmission c, by bits on every row."""
    c8 = (200, 90, 31)
    c = (np.array(c8, np.uint8).astype(F) * T.ONE_OVER_255).astype(F)
    st = T.st_rows(2, 3, seed=2)
    for cls, plain, key, floats, rows_of in (
            ("MatteTextured", "Matte", "reflectance", {}, "matte_scene"),
            ("ThinDielectric", "ThinDielectric", "transmission", {"eta": 1.5, "thickness": 0.4, "transparency": 0.8},
             "thindielectric")):
        rows = R.material_rows(rows_of)
        got = oracle.material_components(_constant_case(cls, c8, floats).blob(), R.VACUUM, np.concatenate([rows, st], 1))
        want = R.oracle_material(plain, dict(floats, **{key: tuple(float(x) for x in c)}), R.VACUUM, rows)
        assert int(want[0, 0:1].view(np.int32)[0]) >= 1
        assert R.same_bits(got, want).all(), cls


# ---------------------------------------------------------------- GPU
def _rows22(rows20, st=None):
    return np.concatenate([rows20, np.zeros((rows20.shape[0], 2), F) if st is None else st], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.MATERIALS))
def test_gpu_shade_material_equals_the_fixture(gpu_device, name):
    """The host material commit, geom_burst and the shade_material switch, then comp_eval and
    comp_sample, against the reference library's recorded answers: through the every-material
    instantiation and through each specialized one that holds the material."""
    cls, parms, medium = R.MATERIALS[name]
    rows, fix = S._material_fixture(name)
    scene, prims = T.Case({}, {}, [(cls, parms, {})]).build(gpu_device)
    for which in _sets(cls, name):
        got = gpu_device.debug_material(scene, prims[0], _rows22(rows), medium, which)
        S._check_material(f"material {name} gpu/{which}", got, fix)
    gpu_device.rtDecRef(scene)


@pytest.mark.gpu
def test_gpu_material_outside_the_named_set_is_refused(gpu_device):
    scene, prims = T.Case({}, {}, [("Mirror", {}, {}), ("Matte", {}, {})]).build(gpu_device)
    rows = _rows22(R.material_rows("mirror_default"))
    with pytest.raises(RuntimeError, match="does not hold"):
        gpu_device.debug_material(scene, prims[0], rows, R.VACUUM, "uber")
    with pytest.raises(RuntimeError, match="unknown material set"):
        gpu_device.debug_material(scene, prims[0], rows, R.VACUUM, "everything")
    # the second primitive is found by its own record, not the first one's
    got = gpu_device.debug_material(scene, prims[1], rows, R.VACUUM, "spheres")
    assert (got[:, 1].view(np.uint32) == 0x1).all() and (got[:, 0].view(np.int32) == 1).all()
    gpu_device.rtDecRef(scene)


def _gpu_lookups(dev, case, w, h, fmt):
    st, want = _expected(w, h, fmt)
    scene, prims = case.build(dev)
    for j in range(4):   # material j + 1: map_d = T through combination j, map_Ks = through combination j + 1
        out = dev.debug_textures(scene, prims[1 + j], st)
        texs = case.materials[1 + j][2]
        for slot, key in enumerate(T.Case.TEX_SLOTS[:5]):
            if key not in texs:
                assert (out[:, slot].view(np.uint32) == 0).all(), (j, key)
                continue
            filt, inv, im = case.textures[texs[key]]
            f, a = case.images[im]
            exp = want[texs[key]] if im == "T" else T.lookup(a, f, filt, inv, st[:, 0], st[:, 1])
            bad = np.where(~R.same_bits(out[:, slot], exp))[0]
            assert bad.size == 0, (j, key, filt, inv, bad[:8].tolist(), st[bad[:2]].tolist(), out[bad[:2], slot].tolist(),
                                   exp[bad[:2]].tolist())
        # slot 0 through the texture table == slot 0 through the descriptor copy in the geometry record
        assert R.same_bits(out[:, 5], out[:, 0]).all(), j
    dev.rtDecRef(scene)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt", IMAGES, ids=image_ids)
def test_gpu_texture_lookup_equals_the_restatement(gpu_device, w, h, fmt):
    """tex_get and tex_get_rec(t0) of the image under test, second in its pool part, through both
    filters with invert off and on, and of its neighbours: == numpy by bits on the 1024 rows."""
    _gpu_lookups(gpu_device, T.lookup_case(w, h, fmt), w, h, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt", [(3, 5, "RGBA8"), (5, 3, "RGB_FLOAT32"), (1, 1, "RGB_FLOAT32"), (1, 4, "RGB8")],
                         ids=["3x5-RGBA8", "5x3-RGB_FLOAT32", "1x1-RGB_FLOAT32", "1x4-RGB8"])
def test_gpu_texture_lookup_of_the_last_image(gpu_device, w, h, fmt):
    """The same with the image under test last in its pool part (a float image: last in the pool)."""
    _gpu_lookups(gpu_device, T.lookup_case(w, h, fmt, last=True), w, h, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_textured_cases()))
def test_gpu_textured_material_equals_the_oracle(gpu_device, name):
    """MatteTextured, Uber, ThinDielectric and Obj over textures: device == oracle under the rules
    above, through the every-material instantiation and every specialized one that holds the class,
    and all those runs bit-identical to one another."""
    case = _textured_cases()[name][0]
    cls = case.materials[0][0]
    rows, want = _textured_rows(name), _textured_oracle(name)
    scene, prims = case.build(gpu_device)
    runs = {which: gpu_device.debug_material(scene, prims[0], rows, R.VACUUM, which) for which in _sets(cls)}
    gpu_device.rtDecRef(scene)
    for which, got in runs.items():
        _check_textured(f"textured {name} gpu/{which}", got, want, strict=name in STRICT)
        assert R.same_bits(got, runs["all"]).all(), f"{which} differs from the every-material instantiation"
