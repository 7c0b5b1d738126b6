"""The float layer between common/math and the integrator, pinned to the reference's own classes.

oracle/_ref/libref_shade.so (make -C oracle ref) is the reference's cameras (PinHoleCamera,
DepthOfFieldCamera, StereoCubeCamera), its 16 BRDF component classes, CompositedBRDF::sample, its
point / spot / directional / distant / triangle lights, Material::shade of its nine texture-free
materials and its SamplerFactory with the B-spline filter, compiled unmodified behind
oracle/ref_shade.cpp. The transcendentals are substituted by yrt_libm.h's in that build (stated
at the top of the driver): everything around them is compared bit for bit.

Three witnesses per case of ROWS rows (tests/ref_shade_cases.py: edge rows, then random rows):
  live      oracle == the library, and the committed fixture == the library (where it is built
            and the CPU is Intel: rcpps / rsqrtps are vendor-specific);
  fixture   oracle == tests/golden/ref_shade_*.npz, on any host;
  gpu       the device probe (k_check_shade: the kernels' own comp_eval / comp_sample /
            set_sample / camera_ray / light_sample) == the fixture.

Comparison rules, none of them a tolerance:
  * words are compared by bits; a NaN equals a NaN of any sign and payload (the instruction set
    chooses those: SSE generates 0xffc00000, gfx950 0x7fc00000);
  * a colour that is exactly zero may differ in the sign of the zero: _mm_dp_ps adds its masked
    fourth lane's +0, so the reference's dot product of a negative-zero vector is +0 (as for
    `dot` in tests/test_ref_pin.py);
  * where the reference's sample is rejected by CompositedBRDF's own rule (colour all zero, or
    pdf <= 0) the direction is unspecified and only colour and pdf are compared. The generator
    asserts that such rows are at most a quarter of a case.
Each test prints how many rows it compared and how many on colour and pdf only.
"""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

import oracle
import ref_shade_cases as R

GOLDEN = Path(__file__).resolve().parent / "golden"
_lib = C.CDLL(str(oracle.REF_SHADE_LIB)) if oracle.REF_SHADE_LIB.exists() else None


def live(fn):
    """Needs the compiled reference and an Intel CPU (rcp / rsqrt take part in every case)."""
    fn = pytest.mark.skipif(_lib is None, reason="oracle/_ref/libref_shade.so not built (make -C oracle ref)")(fn)
    return pytest.mark.skipif(R.cpu_vendor() != "GenuineIntel",
                              reason="rcpps/rsqrtps tables are vendor-specific; the fixture is Intel's")(fn)


@functools.lru_cache(maxsize=None)
def _fixture(stem):
    return np.load(GOLDEN / f"ref_shade_{stem}.npz")


def _want(stem, name, *inputs):
    f = _fixture(stem)
    assert np.array_equal(f[name + ".digest"], R.digest(*inputs)), f"{name}: the fixture belongs to other inputs"
    return f[name]


def _zero_sign_ok(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))
    return word.reshape(a.shape[0], int(np.prod(a.shape[1:]))).all(1)


def _check(label, got, want, colour, direction=None, rejected=None):
    """got / want (rows, words): `colour` columns by bits up to the sign of a zero, `direction`
    columns by bits except in `rejected` rows, every other column by bits."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    n = want.shape[0]
    rej = np.zeros(n, bool) if rejected is None else rejected
    cols = np.ones(want.shape[1], bool)
    cols[colour] = False
    ok = _zero_sign_ok(got[:, colour], want[:, colour])
    if direction is not None:
        cols[direction] = False
        ok &= R.same_bits(got[:, direction], want[:, direction]) | rej
    ok &= R.same_bits(got[:, cols], want[:, cols])
    print(f"{label}: {n} rows compared, {int(rej.sum())} on colour and pdf only, {int(np.isnan(want).sum())} NaN words")
    assert rej.sum() * 4 <= n
    bad = np.where(~ok)[0]
    assert bad.size == 0, (label, bad.size, bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


BRDF_COL, BRDF_DIR = slice(0, 6), slice(6, 9)
SET_COL, SET_DIR = slice(0, 3), slice(3, 6)
LIGHT_COL = slice(0, 3)


def _brdf_inputs(c):
    return [c[k] for k in ("args", "wo", "Ns", "Ng", "Tx", "Ty", "wi", "s")]


def _brdf_rows(out4):
    ev, sa, wi, pdf = out4
    return np.concatenate([ev, sa, wi, pdf[:, None]], 1)


def _set_inputs(c):
    return [c[k] for k in ("kinds", "args", "wo", "frame", "s", "ss")]


def _set_rows(out4):
    col, wi, pdf, typ = out4
    return np.concatenate([col, wi, pdf[:, None], typ.view(np.float32)[:, None]], 1)


def _brdf_fixture(kind):
    c = R.brdf_case(kind)
    return c, _want("brdf0" if kind < 8 else "brdf1", R.KIND_NAMES[kind], *_brdf_inputs(c))


def _set_fixture(name):
    c = R.set_case(name)
    return c, _want("sets", name, *_set_inputs(c))


def _camera_fixture(name):
    typ, parms, px, lens = CAMERAS[name]
    return _want("cameras0" if name.endswith("toe0") else "cameras1", name, R.camera_params(parms), px, lens)


def _light_fixture(name):
    typ, parms, xfm, P, s = LIGHTS[name]
    return _want("lights", name, R.light_params(xfm, parms), P, s)


KINDS = list(range(16))
CAMERAS = R.camera_cases()
LIGHTS = R.light_cases()
kind_ids = [f"{k}_{n}" for k, n in enumerate(R.KIND_NAMES)]


# ---------------------------------------------------------------- live: the compiled reference
@live
@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_brdf_components_equal_the_reference(kind):
    """BRDF::eval and BRDF::sample of the class named at CompKind `kind` (kernels/yrt_shade.h:36-55):
    oracle == library, fixture == library."""
    c, fix = _brdf_fixture(kind)
    ref = _brdf_rows(R.ref_brdf(_lib, kind, c))
    rej = R.rejected(ref[:, 3:6], ref[:, 9])
    _check(f"brdf {R.KIND_NAMES[kind]} oracle", _brdf_rows(R.oracle_brdf(kind, c)), ref, BRDF_COL, BRDF_DIR, rej)
    assert np.array_equal(fix.view(np.uint32), ref.view(np.uint32)), "the fixture is not this library's output"


@live
@pytest.mark.parametrize("name", list(R.SETS))
def test_composited_sample_equals_the_reference(name):
    """CompositedBRDF::sample (compositedbrdf.h:104-166) over the component set a material creates."""
    c, fix = _set_fixture(name)
    ref = _set_rows(R.ref_set_sample(_lib, c))
    _check(f"set {name} oracle", _set_rows(R.oracle_set_sample(c)), ref, SET_COL, SET_DIR,
           R.rejected(ref[:, 0:3], ref[:, 6]))
    assert np.array_equal(fix.view(np.uint32), ref.view(np.uint32)), "the fixture is not this library's output"


@live
@pytest.mark.parametrize("name", list(CAMERAS))
def test_camera_rays_equal_the_reference(name):
    """Camera::ray of the class built from Parms (absent parameters: the class's defaults)."""
    typ, parms, px, lens = CAMERAS[name]
    ref = np.concatenate(R.ref_camera(_lib, typ, parms, px, lens), 1)
    _check(f"camera {name} oracle", np.concatenate(R.oracle_camera(typ, parms, px, lens), 1), ref, slice(0, 0))
    assert np.array_equal(_camera_fixture(name).view(np.uint32), ref.view(np.uint32))


@live
@pytest.mark.parametrize("name", list(LIGHTS))
def test_light_samples_equal_the_reference(name):
    """Light::sample after Light::transform: radiance, direction and pdf (ls.tMax is overwritten by
    the integrator, pathtraceintegrator.cpp:152, and is not part of either side)."""
    typ, parms, xfm, P, s = LIGHTS[name]
    L, wi, pdf = R.ref_light(_lib, typ, parms, xfm, P, s)
    ref = np.concatenate([L, wi, pdf[:, None]], 1)
    L, wi, pdf = R.oracle_light(typ, parms, xfm, P, s)
    _check(f"light {name} oracle", np.concatenate([L, wi, pdf[:, None]], 1), ref, LIGHT_COL)
    assert np.array_equal(_light_fixture(name).view(np.uint32), ref.view(np.uint32))


def _material_fixture(name):
    typ, parms, medium = R.MATERIALS[name]
    rows = R.material_rows(name)
    f = _fixture(R.material_stem(name))
    assert np.array_equal(f[name + ".digest"], R.material_digest(typ, parms, medium, rows))
    return rows, f[name]


def _check_material(label, got, want):
    """(rows, 34) = count, 3 x (type, eval3, sample3, wi3, pdf): the count and the words of absent
    components by bits; of each component the material created, type and pdf by bits, the colours
    up to the sign of a zero, and the direction unless the reference's sample is rejected (at most
    a quarter of the rows of each component, as for every other case)."""
    assert np.array_equal(got[:, 0].view(np.int32), want[:, 0].view(np.int32)), label + ": component counts"
    count = int(want[0, 0:1].view(np.int32)[0])
    assert (want[:, 0].view(np.int32) == count).all() and 1 <= count <= 3
    assert np.array_equal(got[:, 1 + 11 * count:].view(np.uint32), want[:, 1 + 11 * count:].view(np.uint32))
    for k in range(count):
        c = slice(1 + 11 * k, 12 + 11 * k)
        g, w = got[:, c], want[:, c]
        _check(f"{label} component {k}", g, w, slice(1, 7), slice(7, 10), R.rejected(w[:, 4:7], w[:, 10]))


@live
@pytest.mark.parametrize("name", list(R.MATERIALS))
def test_material_components_equal_the_reference(name):
    """Material::shade of the nine texture-free materials (scenes/materials_lights.xml's parameters,
    the defaults, and each constructor branch): how many components, their type flags, and what
    each returns from eval and sample on 1024 rows; oracle == library, fixture == library."""
    typ, parms, medium = R.MATERIALS[name]
    rows, fix = _material_fixture(name)
    ref = R.ref_material(_lib, typ, parms, medium, rows)
    _check_material(f"material {name} oracle", R.oracle_material(typ, parms, medium, rows), ref)
    assert np.array_equal(fix.view(np.uint32), ref.view(np.uint32)), "the fixture is not this library's output"


@pytest.mark.parametrize("name", list(R.MATERIALS))
def test_material_components_equal_the_fixture(name):
    typ, parms, medium = R.MATERIALS[name]
    rows, fix = _material_fixture(name)
    _check_material(f"material {name} oracle/fixture", R.oracle_material(typ, parms, medium, rows), fix)


# ---------------------------------------------------------------- the oracle against the fixtures
@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_brdf_components_equal_the_fixture(kind):
    c, fix = _brdf_fixture(kind)
    _check(f"brdf {R.KIND_NAMES[kind]} oracle/fixture", _brdf_rows(R.oracle_brdf(kind, c)), fix, BRDF_COL, BRDF_DIR,
           R.rejected(fix[:, 3:6], fix[:, 9]))


@pytest.mark.parametrize("name", list(R.SETS))
def test_composited_sample_equals_the_fixture(name):
    c, fix = _set_fixture(name)
    _check(f"set {name} oracle/fixture", _set_rows(R.oracle_set_sample(c)), fix, SET_COL, SET_DIR,
           R.rejected(fix[:, 0:3], fix[:, 6]))


@pytest.mark.parametrize("name", list(CAMERAS))
def test_camera_rays_equal_the_fixture(name):
    typ, parms, px, lens = CAMERAS[name]
    _check(f"camera {name} oracle/fixture", np.concatenate(R.oracle_camera(typ, parms, px, lens), 1),
           _camera_fixture(name), slice(0, 0))


@pytest.mark.parametrize("name", list(LIGHTS))
def test_light_samples_equal_the_fixture(name):
    typ, parms, xfm, P, s = LIGHTS[name]
    L, wi, pdf = R.oracle_light(typ, parms, xfm, P, s)
    _check(f"light {name} oracle/fixture", np.concatenate([L, wi, pdf[:, None]], 1), _light_fixture(name), LIGHT_COL)


@pytest.mark.parametrize("spp,iteration,n1,n2", R.TABLE_SHAPES)
def test_filtered_pixel_samples_equal_the_fixture(spp, iteration, n1, n2):
    """The oracle's B-spline-warped pixel samples (the filter touches dims 0 and 1 only) against
    those of the reference's real SamplerFactory::init (tests/test_ref_pin.py compares every dim
    with the live library)."""
    want = _want("table", f"spp{spp}_it{iteration}_{n1}_{n2}", np.array([spp, 64, iteration, n1, n2], np.int32))
    got = oracle.sample_table(spp, 64, iteration, n1, n2, filter="bspline")
    print(f"sample table spp {spp} iteration {iteration}: {want.size} words compared")
    assert np.array_equal(got[:2].view(np.uint32), want.view(np.uint32))


def test_cases_cover_the_edges():
    """The edge rows the cases promise are there (a check of the generator, not of the renderer)."""
    c = R.brdf_case(0)
    d = (c["wo"] * c["Ns"]).sum(-1)
    assert (d == 0).any() and (d == 1).any() and (d < 0).any() and (np.abs(d[d != 0]).min() <= R.TINY)
    below_ng = ((c["wi"] * c["Ns"]).sum(-1) > 0) & ((c["wi"] * c["Ng"]).sum(-1) < 0)
    above_ng = ((c["wi"] * c["Ns"]).sum(-1) < 0) & ((c["wi"] * c["Ng"]).sum(-1) > 0)
    assert below_ng.any() and above_ng.any()
    assert np.array_equal(c["wi"][-1], R._reflect(c["wo"][-1:], c["Ns"][-1:])[0])
    for v in (0.0, 0.5, float(R.ONE_M)):
        assert (c["s"][:, 0] == np.float32(v)).any() and (c["s"][:, 1] == np.float32(v)).any() and \
            (c["ss"] == np.float32(v)).any()
    assert {0.0, 1.0, 64.0, 1e4, 1e3, 2.0} <= set(R.brdf_args(7, 0)[:, 3].tolist())
    assert (R.brdf_args(9, 0)[:, 9:12] == 0).all(1).any() and (R.brdf_args(0, 0)[:, 1] == 0).any()
    assert {(1.0, 1.0), (1.0, 1.5), (1.5, 1.0)} == set(map(tuple, R.brdf_args(14, 0)[:, 3:5].tolist()))
    faces = {(p["cubeFaceIndex"], p["toeIn"]) for t, p, _, _ in CAMERAS.values() if "stereFalloffAngle" in p}
    assert faces == {(f, t) for f in range(12) for t in (0, 1)}
    assert {p["stereFalloffAngle"] for t, p, _, _ in CAMERAS.values() if "stereFalloffAngle" in p} == {0.0, 30.0, 90.0}


# ---------------------------------------------------------------- the device probe
def _probe_rows(c, kinds, args):
    """k_check_shade's rows (n, 48) and material records (n * nk, 32) for components `kinds` with
    constructor arguments args (n, nk, 16): the component records are the oracle's."""
    n, nk = args.shape[0], len(kinds)
    rows = np.zeros((n, 48), np.float32)
    for k, at in (("wo", 0), ("Ns", 3), ("Ng", 6), ("Tx", 9), ("Ty", 12), ("wi", 15), ("s", 18)):
        rows[:, at:at + c[k].shape[1]] = c[k]
    rows[:, 20] = c["ss"]
    rows[:, 21] = np.full(n, nk, np.int32).view(np.float32)
    mats = np.zeros((n * nk, 32), np.float32)  # GpuMaterial: 8 int32 words, then p[24]
    for j, kind in enumerate(kinds):
        comp = oracle.brdf_comps(kind, args[:, j])
        at = 24 + 8 * j
        rows[:, at] = np.full(n, kind, np.int32).view(np.float32)
        rows[:, at + 1:at + 7] = comp
        if kind in (9, 10, 11):  # conductors read eta, k from their material record (p[3..8])
            ids = (np.arange(n, dtype=np.int32) * nk + j)
            rows[:, at + 6] = ids.view(np.float32)
            mats[ids, 8 + 3:8 + 9] = args[:, j, 6:12]
    return rows, mats


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=kind_ids)
def test_gpu_brdf_components_equal_the_fixture(gpu_device, kind):
    c, fix = _brdf_fixture(kind)
    rows, mats = _probe_rows(c, [kind], c["args"][:, None, :])
    out = gpu_device.debug_shade(0, rows, mats)
    _check(f"brdf {R.KIND_NAMES[kind]} gpu", out[:, :10], fix, BRDF_COL, BRDF_DIR, R.rejected(fix[:, 3:6], fix[:, 9]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.SETS))
def test_gpu_composited_sample_equals_the_fixture(gpu_device, name):
    c, fix = _set_fixture(name)
    rows, mats = _probe_rows(c, R.SETS[name], c["args"])
    out = gpu_device.debug_shade(1, rows, mats)
    _check(f"set {name} gpu", out[:, :8], fix, SET_COL, SET_DIR, R.rejected(fix[:, 0:3], fix[:, 6]))


def _set_parms(dev, h, parms, kinds):
    for k, v in parms.items():
        v = np.atleast_1d(np.asarray(v, np.float32))
        if kinds.get(k) == "xfm":
            dev.rtSetTransform(h, k, v)
        elif kinds.get(k) == "int":
            dev.rtSetInt1(h, k, int(v[0]))
        elif kinds.get(k) == "bool":
            dev.rtSetBool1(h, k, bool(v[0]))
        elif v.size == 3:
            dev.rtSetFloat3(h, k, *v)
        else:
            dev.rtSetFloat1(h, k, v[0])
    dev.rtCommit(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CAMERAS))
def test_gpu_camera_rays_equal_the_fixture(gpu_device, name):
    typ, parms, px, lens = CAMERAS[name]
    cam = gpu_device.rtNewCamera(typ)
    _set_parms(gpu_device, cam, parms, {"local2world": "xfm", "cubeFaceIndex": "int", "toeIn": "bool"})
    rows = np.zeros((px.shape[0], 48), np.float32)
    rows[:, 0:2], rows[:, 18:20] = px, lens
    out = gpu_device.debug_shade(2, rows, obj=cam)
    gpu_device.rtDecRef(cam)
    _check(f"camera {name} gpu", out[:, :6], _camera_fixture(name), slice(0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LIGHTS))
def test_gpu_light_samples_equal_the_fixture(gpu_device, name):
    typ, parms, xfm, P, s = LIGHTS[name]
    light = gpu_device.rtNewLight(typ)
    _set_parms(gpu_device, light, parms, {})
    prim = gpu_device.rtNewLightPrimitive(light, None, xfm)
    rows = np.zeros((P.shape[0], 48), np.float32)
    rows[:, 0:3], rows[:, 18:20] = P, s
    rows[:, 3:9] = np.array([0, 0, 1, 0, 0, 1], np.float32)
    out = gpu_device.debug_shade(3, rows, obj=prim)
    gpu_device.rtDecRef(prim)
    gpu_device.rtDecRef(light)
    _check(f"light {name} gpu", out[:, :7], _light_fixture(name), LIGHT_COL)
