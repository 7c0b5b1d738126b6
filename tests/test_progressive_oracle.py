"""Progressive frames on the CPU side: the host sampler's tables at non-zero iterations against
the oracle's (which tests/test_ref_pin.py pins to the reference at the same iterations), and the
oracle's own accumulation (oracle.render(..., iteration, accu)) against float64 arithmetic.
The device's progressive frames are compared with these in tests/test_progressive.py."""
import numpy as np
import pytest

import oracle
import yrt
from helpers import c1_args
from progressive_ref import check_mean, oracle_frame, oracle_sequence

# (spp, iteration): the last iteration of a 64-sample chunk, the first and second of the next one
# (spp 1: 63, 64, 65; spp 16: 3, 4; spp 32: 2; spp 64: every iteration is a chunk), a chunk larger
# than 64 (spp 256), and spp values the factory rounds up to a power of two (3 -> 4, 33 -> 64)
ITERATIONS = [(1, 1), (1, 63), (1, 64), (1, 65), (16, 3), (16, 4), (32, 2), (64, 1), (256, 2), (3, 5), (33, 2)]


@pytest.mark.parametrize("dims", [(2, 3), (10, 11)], ids=["d2", "d10"])
@pytest.mark.parametrize("filter", ["bspline", "none"])
@pytest.mark.parametrize("spp,iteration", ITERATIONS)
def test_host_sample_table_equals_oracle_at_iteration(spp, iteration, filter, dims):
    """build_sample_table (csrc/device/sampler.cpp) against the oracle's table, bit for bit."""
    sets = 64
    a =yrt.sample_table(spp, sets, iteration, dims[0], dims[1], filter)
    b = oracle.sample_table(spp, sets, iteration, dims[0], dims[1], filter)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # and the iteration matters: the same request at iteration 0 is another table
    assert not np.array_equal(a, oracle.sample_table(spp, sets, 0, dims[0], dims[1], filter))


W = 32
SPP = 16
K = 6  # iteration 4 opens the second chunk at spp 16


@pytest.fixture(scope="module")
def c1_blob(host_device):
    s = yrt.Session(c1_args(W, SPP) + ["-fb", "RGB_FLOAT32"], device=host_device)
    blob = s.export_frame()
    s.close()
    return blob


def test_iteration_zero_without_accu_is_the_old_entry_point(c1_blob):
    """iteration=0, accu=None goes through oracle_render as before; the new entry point gives the
    same frame for it, and a first accumulated frame shows the same bits as a frame alone."""
    old = oracle.render(c1_blob, W, W, 1.0)[0]
    accu = np.zeros((W, W, 4), np.float32)
    first = oracle.render(c1_blob, W, W, 1.0, iteration=0, accu=accu)[0]
    assert np.array_equal(old.view(np.uint32), first.view(np.uint32))
    assert np.array_equal(accu[..., 3], np.full((W, W), SPP, np.float32))
    # the sums are what the display divides: L = accu.xyz, display = L * rcp(spp)
    rs = oracle.vecmath("rcp", np.array([SPP], np.float32))[0]
    assert np.array_equal((accu[..., :3] * rs).view(np.uint32), first.view(np.uint32))
    with pytest.raises(ValueError):
        oracle.render(c1_blob, W, W, 1.0, accu=np.zeros((W, W, 3), np.float32))


def test_iterations_differ(c1_blob):
    """Iteration k's frame is not iteration 0's: k = 1 (another offset into the chunk) and k = 4
    (the first iteration of the next chunk, another seed)."""
    f0 = oracle_frame(c1_blob, W, W, 1.0, 0)
    for k in (1, 64 // SPP):
        fk = oracle_frame(c1_blob, W, W, 1.0, k)
        assert np.isfinite(fk).all()
        assert (fk != f0).mean() > 0.5, k
    assert (oracle_frame(c1_blob, W, W, 1.0, 1) != oracle_frame(c1_blob, W, W, 1.0, 64 // SPP)).mean() > 0.5


def test_oracle_accumulation_equals_the_float64_mean(c1_blob):
    """After every one of K accumulated frames, the display against the float64 mean of the same
    iterations rendered alone, within progressive_ref.mean_bound (derived there)."""
    shown = oracle_sequence(c1_blob, W, W, 1.0, K)
    singles = [oracle_frame(c1_blob, W, W, 1.0, k) for k in range(K)]
    for n in range(1, K + 1):
        check_mean(shown[n - 1], singles[:n])
    # the bound tells a wrong weight from a right one: K frames divided by K + 1 miss it
    with pytest.raises(AssertionError):
        check_mean(shown[K - 1] * np.float32(K / (K + 1)), singles)
