"""Progressive frames on the device: rtRenderFrame(..., accumulate=1) after every call against the
oracle's restatement of the same calls (tests/progressive_ref.py), bit for bit.

rtRenderFrame(..., accumulate=1) is the reference's interactive mode: each call raises the
renderer's iteration (renderers/integratorrenderer.cpp:63-69), builds that iteration's sample table
(samplers/sampler.cpp:85-95, with the precomputed light samples) and adds the frame into the swap
chain's accumulation buffer (api/framebuffer.h:289-304, api/swapchain.h:44); the display is the
running average, then gamma and the 8-bit store. Pinned here: the tables of iterations >= 1 as the
kernels see them (dims, direction terms, light slots, chunk and offset), the average's arithmetic,
the restart by accumulate=0, the frame-cache eviction, and that the accumulation belongs to the
framebuffer: a new framebuffer starts from a cleared buffer, two framebuffers refined in turn do
not see each other, and a multi-frame job in between leaves a refined framebuffer alone.
"""
import numpy as np
import pytest

import yrt
from helpers import SCENES, c1_args, c2_args, parity
from progressive_ref import check_mean, oracle_frame, oracle_sequence

pytestmark = pytest.mark.gpu


class Progressive:
    """A command-line session whose framebuffer is refined call by call through the C ABI."""

    def __init__(self, dev, args, face=-1, fmt="RGB_FLOAT32"):
        self.dev, self.fmt = dev, fmt
        self.s = yrt.Session(args + ["-fb", fmt], device=dev)
        self.i = self.s.info()
        self.cam = self.s.camera(face)
        self.W, self.H, self.gamma = self.i["width"], self.i["height"], self.i["gamma"]
        self.blob = self.s.export_frame(camera=self.cam)

    def frame(self, accumulate=1, framebuffer=None):
        fb = framebuffer or self.i["framebuffer"]
        self.dev.rtRenderFrame(self.i["renderer"], self.cam, self.i["scene"], self.i["tonemapper"], fb, accumulate)
        return self.dev.framebuffer_array(fb, self.W, self.H, self.fmt)

    def oracle(self, count):
        """The display after each of `count` progressive frames from a new or restarted state."""
        return oracle_sequence(self.blob, self.W, self.H, self.gamma, count)

    def close(self):
        self.s.close()


def _same(img, ref, what):
    try:
        parity(img, ref, 0.0, mad_rel=None, exact=True)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _hdri_args():
    from test_gpu_parity import _hdri_scene
    return ["-i", str(_hdri_scene()), "-c", str(SCENES / "test_stereo_view.ecs"), "-size", "32", "32", "-spp", "4",
            "-stereo"]


# name -> (session arguments, cube face, frames). C2 at 16 spp: iteration 4 opens the second
# 64-sample chunk. The HDRI light's precomputed samples are rebuilt per iteration; the thin lens
# reads the lens dimensions and the moving scene the time dimension of every iteration's table.
SEQUENCES = {
    "C1": (lambda: c1_args(64, 1), -1, 5),
    "C2": (lambda: c2_args(32, 16), -1, 6),
    "hdri": (_hdri_args, 0, 3),
    "dof": (lambda: ["-c", str(SCENES / "materials_lights.ecs"), "-size", "24", "18", "-spp", "4", "-radius", "6"],
            -1, 3),
    "motion": (lambda: ["-c", str(SCENES / "samples" / "sphere_motion.ecs"), "-size", "40", "40", "-spp", "4"], -1, 3),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_every_progressive_frame_equals_the_oracle(gpu_device, name):
    args, face, K = SEQUENCES[name]
    p = Progressive(gpu_device, args(), face)
    ref = p.oracle(K)
    for k in range(K):
        _same(p.frame(1), ref[k], f"{name} after call {k}")
    assert not np.array_equal(ref[0], ref[1])
    p.close()


def test_tone_mapping_applies_to_the_accumulated_value(gpu_device):
    """Gamma 2.2 on the running average, as floats and as the truncated bytes of RGB8."""
    K = 3
    args = c1_args(64, 1) + ["-gamma", "2.2"]
    pf, p8 = Progressive(gpu_device, args), Progressive(gpu_device, args, fmt="RGB8")
    assert pf.gamma == np.float32(2.2) and p8.gamma == pf.gamma
    ref, ref_bytes = pf.oracle(K), p8.oracle(K)
    for k in range(K):
        _same(pf.frame(1), ref[k], f"RGB_FLOAT32 after call {k}")
        img8 = p8.frame(1).astype(np.int32)
        ref8 = np.clip(ref_bytes[k] * 255.0, 0, 255).astype(np.int32)
        assert np.array_equal(img8, ref8), (k, int(np.abs(img8 - ref8).max()))
    # the gamma is applied after the average: the average of gamma-mapped frames is another image
    lin = oracle_sequence(pf.blob, 64, 64, 1.0, K)
    assert not np.array_equal(ref[K - 1], lin[K - 1])
    pf.close()
    p8.close()


def test_accumulated_frames_equal_the_float64_mean(gpu_device):
    """The device's display after n accumulated frames against the float64 mean of iterations
    0..n-1 rendered alone by the oracle, within progressive_ref.mean_bound (derived there, not
    tuned): the weights and the order of the sums, independent of the oracle's own accumulation."""
    K = 6
    p = Progressive(gpu_device, c1_args(32, 16) + ["-gamma", "1"])
    assert p.gamma == 1.0
    singles = [oracle_frame(p.blob, 32, 32, 1.0, k) for k in range(K)]
    for n in range(1, K + 1):
        check_mean(p.frame(1), singles[:n])
    p.close()


def test_restart(gpu_device):
    """accumulate=0 after K progressive frames: the iteration-0 frame again, and the next
    accumulate=1 call is the second frame of a new sequence."""
    K = 4
    p = Progressive(gpu_device, c2_args(32, 4))
    ref = p.oracle(K)
    for k in range(K):
        _same(p.frame(1), ref[k], f"call {k}")
    _same(p.frame(0), ref[0], "accumulate=0 after the sequence")
    _same(p.frame(1), ref[1], "the first accumulate=1 after the restart")
    _same(p.frame(1), ref[2], "the second accumulate=1 after the restart")
    p.close()


def test_frame_cache_eviction(gpu_device):
    """More iterations than a context keeps sample tables for (GpuCtx::kMaxFrameCaches = 16): every
    frame is still the oracle's, and accumulate=0 rebuilds the evicted iteration-0 table."""
    K = 20
    p = Progressive(gpu_device, c1_args(32, 1))
    ref = p.oracle(K)
    first = None
    for k in range(K):
        img = p.frame(1)
        first = img if first is None else first
        _same(img, ref[k], f"call {k}")
    again = p.frame(0)
    assert np.array_equal(again, first)
    _same(again, ref[0], "accumulate=0 after 20 iterations")
    p.close()


def test_fresh_framebuffer_starts_clean(gpu_device):
    """A new framebuffer's first frame with accumulate=1 is that frame alone (the reference's
    cleared AccuBuffer), whatever was accumulated on the device before at the same size."""
    a = Progressive(gpu_device, c1_args(64, 1))
    ra = a.oracle(4)
    for k in range(3):  # accumulate=0 first: A's sums are defined whatever the device held before
        _same(a.frame(1 if k else 0), ra[k], f"A call {k}")
    b = Progressive(gpu_device, c2_args(64, 1))
    first = b.frame(1)
    _same(first, b.oracle(1)[0], "B's first frame, accumulate=1")
    assert np.array_equal(first, b.frame(0)), "B's accumulate=1 first frame differs from its accumulate=0 frame"
    _same(a.frame(1), ra[3], "A call 3, after B's frames")
    a.close()
    b.close()


@pytest.mark.parametrize("first", [0, 1], ids=["restarted", "new"])
@pytest.mark.parametrize("shards", [1, 2])
def test_two_framebuffers_interleaved(gpu_device, shards, first):
    """Two framebuffers of one size refined in turn (A, B, A, B, A, B): each shows its own
    sequence. shards = 2: a device of two logical shards of GPU 0, each keeping the sums of its
    own tiles. first: the first call's accumulate flag, a restart or a new framebuffer's frame."""
    dev = gpu_device if shards == 1 else yrt.Device(devices=[0, 0])
    try:
        a, b = Progressive(dev, c1_args(32, 4)), Progressive(dev, c2_args(32, 4))
        ra, rb = a.oracle(3), b.oracle(3)
        for k in range(3):
            _same(a.frame(1 if k else first), ra[k], f"A call {k}")
            _same(b.frame(1 if k else first), rb[k], f"B call {k}")
        a.close()
        b.close()
    finally:
        if shards != 1:
            dev.close()


def test_multi_frame_job_in_between(gpu_device):
    """A multi-frame job (rtRenderFrames) between two progressive frames of another framebuffer of
    the same size leaves that framebuffer's accumulation alone. The job's own framebuffers hold no
    accumulation afterwards: accumulate=1 on one of them is refused until a frame
    with accumulate=0 has been rendered into it."""
    dev = gpu_device
    a, b = Progressive(dev, c1_args(32, 4)), Progressive(dev, c2_args(32, 4))
    ra, rb = a.oracle(3), b.oracle(2)
    for k in range(2):
        _same(a.frame(1 if k else 0), ra[k], f"A call {k}")
    fbs = [dev.rtNewFrameBuffer("RGB_FLOAT32", 32, 32) for _ in range(2)]
    try:
        dev.rtRenderFrames(b.i["renderer"], [b.cam, b.cam], b.i["scene"], b.i["tonemapper"], fbs, 0)
        for k, fb in enumerate(fbs):
            _same(dev.framebuffer_array(fb, 32, 32, "RGB_FLOAT32"), rb[0], f"the job's frame {k}")
        _same(a.frame(1), ra[2], "A call 2, after the job")
        with pytest.raises(RuntimeError, match="accumulate"):
            dev.rtRenderFrames(b.i["renderer"], [b.cam, b.cam], b.i["scene"], b.i["tonemapper"], fbs, 1)
        with pytest.raises(RuntimeError, match="multi-frame job"):
            b.frame(1, framebuffer=fbs[0])
        # the refusal changed nothing: accumulate=0 starts the framebuffer's own sequence
        _same(b.frame(0, framebuffer=fbs[0]), rb[0], "the job's framebuffer, accumulate=0")
        _same(b.frame(1, framebuffer=fbs[0]), rb[1], "the job's framebuffer, accumulate=1")
    finally:
        for fb in fbs:
            dev.rtDecRef(fb)
        a.close()
        b.close()
