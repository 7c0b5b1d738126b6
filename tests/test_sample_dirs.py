"""The direction-term table (kernels/k_sample_dirs.h): k_shade loads (cos 2πu, sin 2πu, √v, √(1 − v))
of a 2-D sample from a table filled once per uploaded sample table instead of evaluating the
terms per vertex. The table must hold the bits the per-vertex evaluation produced."""
import os
import subprocess
import sys

import numpy as np
import pytest

import yrt
from helpers import ROOT, SCENES

pytestmark = pytest.mark.gpu

SPP, SETS, DEPTH = 4, 2, 3  # 1 + DEPTH = 4 slots of SETS * SPP = 8 records


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cache(gpu_device):
    dims, dirs = gpu_device.debug_sample_dirs(SPP, SETS, 0, DEPTH, 1 + DEPTH)
    return dims, dirs


def test_table_shape_and_layout(cache):
    dims, dirs = cache
    assert dims.shape == (5 + DEPTH + 2 * (1 + DEPTH), SETS * SPP)
    assert dirs.shape == (1 + DEPTH, SETS * SPP, 4)
    assert np.array_equal(dims, yrt.sample_table(SPP, SETS, 0, DEPTH, 1 + DEPTH))


def test_table_equals_the_per_vertex_terms(gpu_device, cache):
    """Every entry of a frame cache's table, read back from the device, against the probe kernel
    that spells the four terms out from the same (u, v) of the dims table: bit for bit."""
    dims, dirs = cache
    u = dims[5 + DEPTH::2]   # [slot][record]
    v = dims[5 + DEPTH + 1::2]
    assert u.shape == v.shape == dirs.shape[:2]
    want = gpu_device.debug_dir_terms(0, u, v).reshape(dirs.shape)
    assert np.array_equal(_bits(dirs), _bits(want))
    # and the terms are what their names say (float64 reference; the square roots are exact)
    phi = 2.0 * np.pi * u.astype(np.float64)
    assert np.abs(dirs[..., 0] - np.cos(phi)).max() < 1e-6 and np.abs(dirs[..., 1] - np.sin(phi)).max() < 1e-6
    assert np.array_equal(_bits(dirs[..., 2]), _bits(np.sqrt(v)))
    assert np.array_equal(_bits(dirs[..., 3]), _bits(np.sqrt(np.float32(1.0) - v)))


def test_table_kernel_on_quadrant_boundaries_and_range_ends(gpu_device, cache):
    """The table's kernel against the probe on records injected into the cache's rows: u exactly on
    the quadrant boundaries, v = 0 and the largest float below 1."""
    dims, _ = cache
    u = dims[5 + DEPTH::2].ravel().copy()
    v = dims[5 + DEPTH + 1::2].ravel().copy()
    below1 = np.nextafter(np.float32(1.0), np.float32(0.0))
    edge_u = np.array([0.0, 0.25, 0.5, 0.75], np.float32)
    edge_v = np.array([0.0, below1], np.float32)
    uu, vv = np.meshgrid(edge_u, edge_v, indexing="ij")
    k = uu.size
    u[:k], v[:k] = uu.ravel(), vv.ravel()        # boundary u with boundary v
    u[k:k + 4] = edge_u                          # boundary u with a table v
    v[k + 4:k + 6] = edge_v                      # table u with boundary v
    got = gpu_device.debug_dir_terms(1, u, v)
    want = gpu_device.debug_dir_terms(0, u, v)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got[:k:2, 2], np.zeros(4, np.float32)) and np.array_equal(got[:k:2, 3], np.ones(4, np.float32))
    assert np.array_equal(_bits(got[1:k:2, 2]), _bits(np.full(4, np.sqrt(below1), np.float32)))
    assert np.abs(got[:k, 0] - np.repeat([1.0, 0.0, -1.0, 0.0], 2)).max() < 1e-6
    assert np.abs(got[:k, 1] - np.repeat([0.0, 1.0, 0.0, -1.0], 2)).max() < 1e-6


FRAME_ARGS = ["-c", str(SCENES / "materials_lights.ecs"), "-size", "32", "32", "-spp", "4", "-depth", "3",
              "-fb", "RGB_FLOAT32"]
# a build of the device library without the table (the commit before it, or any build that evaluates
# the terms per vertex), selected in a child process with YRT_LIB_DIR
NO_TABLE_LIB = ROOT / "yulio-raytracer_amd" / "lib_variants" / "no_sample_dirs"
CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np
import yrt
dev = yrt.Device(0)
s = yrt.Session({args!r}, device=dev)
np.save({out!r}, s.render())
s.close()
dev.close()
"""


def test_frame_equals_a_build_without_the_table(gpu_device, tmp_path):
    """scenes/materials_lights.xml (Lambertian, layer, microfacet, anisotropic and specular
    samplers; dome, distant and point lights) at 32 x 32, 4 spp, depth 3: byte-equal to the frame
    of a library that evaluates the terms per vertex."""
    if not (NO_TABLE_LIB / "libdevice_singleray_mi355x.so").exists():
        pytest.skip(f"no build without the table at {NO_TABLE_LIB}")
    out = tmp_path / "frame.npy"
    code = CHILD.format(root=str(ROOT), pkg=str(ROOT / "yulio-raytracer_amd"), args=FRAME_ARGS, out=str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120,
                   env=dict(os.environ, YRT_LIB_DIR=str(NO_TABLE_LIB)))
    ref = np.load(out)
    s = yrt.Session(FRAME_ARGS, device=gpu_device)
    img = s.render()
    s.close()
    assert img.dtype == ref.dtype and img.shape == ref.shape
    assert img.tobytes() == ref.tobytes()
    assert np.isfinite(img).all() and img.mean() > 0.01
