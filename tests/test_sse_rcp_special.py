"""yrt_rcpps / yrt_rsqrtps (common/yrt_sse_rcp.h) outside the normal range and at the table
midpoints: the device's form (the hardware estimates taken directly, which leaves zero, subnormal,
huge, inf and NaN inputs to the instruction) against the host's (IEEE division and square root
with an explicit select per case), bit for bit; and the host's against the committed Intel tables.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from test_sse_rcp import _bits, _expect_rcpps, _expect_rsqrtps

SPECIAL = np.array([
    0x00000000, 0x80000000,                          # +-0
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # the smallest and largest subnormals
    0x00800000, 0x80800000,                          # 2^-126
    0x7E800000, 0xFE800000,                          # 2^126: the first input whose estimate flushes to zero
    0x7E7FFFFF, 0x7E800001,                          # its neighbours
    0x7F000000, 0xFF000000,                          # 2^127
    0x7F7FFFFF, 0xFF7FFFFF,                          # the largest finite
    0x7F800000, 0xFF800000,                          # +-inf
    0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FFFFFFF,  # quiet NaNs, payload in the low bits too
    0x7F800001, 0xFF800001, 0x7FA00FFF, 0x7FBFFFFF,  # signalling NaNs
    0xBF800000,                                      # -1 (rsqrtps: the default NaN)
    0x3F800000, 0x40000000, 0x40400000,              # 1, 2, 3
], np.uint32)
_i = np.arange(2048, dtype=np.uint32)
RCP_MID = 0x3F800000 | (_i << 12) | 0x800                       # the 2048 rcpps interval midpoints
RSQ_MID = 0x3F800000 + (_i << 13) + 0x1000                      # 2 x 1024: exponent parity, 10 bits
INPUTS = np.concatenate([SPECIAL, RCP_MID, RSQ_MID]).astype(np.uint32)


def _host(fn, u):
    return _bits(oracle.vecmath(fn, u.view(np.float32)))


def test_host_emulation_on_the_special_inputs():
    x = INPUTS.view(np.float32)
    assert np.array_equal(_host("rcpps", INPUTS), _expect_rcpps(x))
    assert np.array_equal(_host("rsqrtps", INPUTS), _expect_rsqrtps(x))


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name", [(3, "rcpps"), (4, "rsqrtps")])
def test_device_equals_host_on_the_special_inputs(gpu_device, fn, name):
    from yrt import _native as N
    io = np.concatenate([[INPUTS.size], INPUTS]).astype(np.uint64)
    assert N.dev.yrtDebugCheckMath(gpu_device.h, fn, io.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, gpu_device.error()
    got, want = io[1:].astype(np.uint32), _host(name, INPUTS)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(INPUTS[k]), hex(got[k]), hex(want[k])) for k in bad[:8]]
