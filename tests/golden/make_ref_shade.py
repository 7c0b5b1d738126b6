"""Writes tests/golden/ref_shade_*.npz: what the reference's own shading classes return.

    make -C oracle ref && python tests/golden/make_ref_shade.py

oracle/_ref/libref_shade.so is the reference's cameras, BRDF components, CompositedBRDF and
lights, compiled unmodified behind oracle/ref_shade.cpp (whose header states the libm
substitution). This script runs it on the input sets of tests/ref_shade_cases.py and records
the outputs: data the reference's code wrote while running. The inputs are regenerated from seeds
by that module; each case stores a checksum of them, so the fixture says which inputs it belongs
to. tests/test_ref_shade.py compares the oracle and the device probe with these files on any
host, and the files with the live library where it is built.

rcp / rsqrt go through the executing CPU's rcpps / rsqrtps, whose tables are vendor-specific
(tests/golden/sse_rcp_tables.json is Intel's), so this refuses to run on another vendor's CPU.
A rejected sample (CompositedBRDF's own rule: colour all zero or pdf <= 0) leaves the direction
unspecified; the comparison skips the direction of those rows, which may be at most a quarter of
any case (of each component a material creates, for the material cases). That holds for the
reference alone and is asserted here.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(HERE.parent)]

import oracle  # noqa: E402
import ref_shade_cases as R  # noqa: E402

LIMIT = 606336  # the largest fixture committed before these (sample_table_spp64_d10.npy)


def record(lib):
    """file stem -> {array name: array}"""
    files = {"brdf0": {}, "brdf1": {}, "sets": {}, "cameras0": {}, "cameras1": {}, "lights": {}}  # and mat_*, table
    for kind, name in enumerate(R.KIND_NAMES):
        c = R.brdf_case(kind)
        ev, sa, wi, pdf = R.ref_brdf(lib, kind, c)
        rej = R.rejected(sa, pdf)
        assert rej.sum() * 4 <= R.ROWS, (name, int(rej.sum()))
        f = files["brdf0" if kind < 8 else "brdf1"]
        f[name] = np.concatenate([ev, sa, wi, pdf[:, None]], 1)
        f[name + ".digest"] = R.digest(*[c[k] for k in ("args", "wo", "Ns", "Ng", "Tx", "Ty", "wi", "s")])
    for name in R.SETS:
        c = R.set_case(name)
        col, wi, pdf, typ = R.ref_set_sample(lib, c)
        rej = R.rejected(col, pdf)
        assert rej.sum() * 4 <= R.ROWS, (name, int(rej.sum()))
        files["sets"][name] = np.concatenate([col, wi, pdf[:, None], typ.view(np.float32)[:, None]], 1)
        files["sets"][name + ".digest"] = R.digest(*[c[k] for k in ("kinds", "args", "wo", "frame", "s", "ss")])
    for name, (typ, parms, px, lens) in R.camera_cases().items():
        org, dir_ = R.ref_camera(lib, typ, parms, px, lens)
        f = files["cameras0" if name.endswith("toe0") else "cameras1"]
        f[name] = np.concatenate([org, dir_], 1)
        f[name + ".digest"] = R.digest(R.camera_params(parms), px, lens)
    for name, (typ, parms, xfm, P, s) in R.light_cases().items():
        L, wi, pdf = R.ref_light(lib, typ, parms, xfm, P, s)
        files["lights"][name] = np.concatenate([L, wi, pdf[:, None]], 1)
        files["lights"][name + ".digest"] = R.digest(R.light_params(xfm, parms), P, s)
    # Material::shade: one file per material class, every row kept
    for name, (typ, parms, medium) in R.MATERIALS.items():
        rows = R.material_rows(name)
        out = R.ref_material(lib, typ, parms, medium, rows)
        count = int(out[0, 0:1].view(np.int32)[0])
        assert (out[:, 0].view(np.int32) == count).all(), name
        for k in range(count):
            c = out[:, 1 + 11 * k:12 + 11 * k]
            rej = R.rejected(c[:, 4:7], c[:, 10])
            assert rej.sum() * 4 <= R.ROWS, (name, k, int(rej.sum()))
        f = files.setdefault(R.material_stem(name), {})
        f[name] = out
        f[name + ".digest"] = R.material_digest(typ, parms, medium, rows)
    # the filtered sample tables: the B-spline filter warps the pixel dims (0, 1) only
    files["table"] = {}
    for spp, iteration, n1, n2 in R.TABLE_SHAPES:
        t = R.ref_sample_table(lib, spp, 64, iteration, n1, n2, True)
        plain = R.ref_sample_table(lib, spp, 64, iteration, n1, n2, False)
        assert np.array_equal(t[2:].view(np.uint32), plain[2:].view(np.uint32))
        name = f"spp{spp}_it{iteration}_{n1}_{n2}"
        files["table"][name] = t[:2]
        files["table"][name + ".digest"] = R.digest(np.array([spp, 64, iteration, n1, n2], np.int32))
    return files


def main():
    if R.cpu_vendor() != "GenuineIntel":
        sys.exit("make_ref_shade.py: the fixtures record an Intel CPU's rcpps / rsqrtps; this CPU is " + R.cpu_vendor())
    lib = C.CDLL(str(oracle.REF_SHADE_LIB))
    for stem, arrays in record(lib).items():
        path = HERE / f"ref_shade_{stem}.npz"
        np.savez_compressed(path, **arrays)
        size = path.stat().st_size
        assert size < LIMIT, (path.name, size)
        print(f"{path.name}: {len(arrays) // 2} cases, {size} bytes")


if __name__ == "__main__":
    main()
