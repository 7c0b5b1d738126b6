"""bench.py's launch contract (task: `bench.py --gpus N` measures N GPUs or fails).

CPU: a rank count from a launcher that disagrees with --gpus exits non-zero before any GPU or
torch work. GPU: `bench.py --gpus 2` without a launcher starts its own two ranks
(torch.distributed.run children; gloo rehearsal on the one GPU) and rank 0's line says so; a
plain one-GPU run does only the timed steps and --dump-outputs writes their last frame."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT


def _bench(args, env_extra, timeout):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "YRT_BENCH_LAUNCHER"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=env)


@pytest.mark.parametrize("world,gpus", [("3", "2"), ("1", "2"), ("2", "1")])
def test_world_size_must_match_gpus(world, gpus):
    r = _bench(["--gpus", gpus], {"WORLD_SIZE": world, "RANK": "0", "LOCAL_RANK": "0"}, 60)
    assert r.returncode != 0
    assert f"WORLD_SIZE={world} but --gpus {gpus}" in r.stderr


def test_gpus_must_be_positive():
    r = _bench(["--gpus", "0"], {}, 60)
    assert r.returncode != 0 and "--gpus 0" in r.stderr


@pytest.mark.parametrize("args,msg", [(["--stereo-frames", "1"], "--full"), (["--steps", "0"], "--steps")])
def test_rejected_arguments(args, msg):
    """The stereo cubemap is a --full leg (asking for it in a plain run is an error, not silently
    dropped), and a run times at least one step."""
    r = _bench(["--gpus", "1"] + args, {}, 60)
    assert r.returncode != 0 and msg in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_last_frame(tmp_path, gpu_device):
    """A plain run (no --full) times exactly --steps frames, carries none of the --full legs, and
    --dump-outputs writes what a caller of the timed path receives: the frame of the last step
    equals the same workload rendered here through the session, byte for byte (same seeded
    inputs in another process), and the ray counts are that frame's."""
    import numpy as np
    import yrt
    from helpers import c3_args
    r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "96", "--spp", "4",
                "--dump-outputs", str(tmp_path / "out")], {}, 240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["cpu_baseline"] is None and line["stereo_cubemap"] is None and not line["roofline"]["visits"]
    s = yrt.Session(c3_args(96, 4), device=gpu_device)
    ref = s.render()
    st = gpu_device.render_stats()
    s.close()
    frame = np.load(tmp_path / "out" / "frame.npy")
    rays = np.load(tmp_path / "out" / "ray_counts.npy")
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["frame.npy", "ray_counts.npy"]
    assert frame.dtype == np.float32 and frame.shape == ref.shape
    assert np.array_equal(frame, ref.astype(np.float32))
    assert rays.dtype == np.float64 and rays.tolist() == [st["raysClosest"], st["raysShadow"]]
    # --steps sets the number of timed frames: the line's counts are two frames' worth
    assert line["rays_closest"] == 2 * st["raysClosest"] and line["rays_shadow"] == 2 * st["raysShadow"]


@pytest.mark.gpu
def test_gpus_two_without_launcher(tmp_path):
    """The driver's `python bench.py --gpus 2 --full` (no torchrun): two ranks render, the
    cubemap gather is bit-exact against rank 0's one-GPU render."""
    r = _bench(["--gpus", "2", "--full", "--steps", "1", "--warmup", "0", "--size", "128", "--spp", "4", "--capture", "0",
                "--no-cpu-baseline", "--stereo-size", "64", "--stereo-spp", "2"], {"YRT_DIST_BACKEND": "gloo"}, 240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    line = json.loads(lines[0])
    assert line["ranks"] == 2 and line["launcher"].startswith("bench.py --gpus")
    assert line["stereo_cubemap"]["gather_check"] == "bit_exact"
    # the N > 1 diagnosis: each rank's render and gather time, max / mean / min
    for pr in (line["per_rank"], line["stereo_cubemap"]["per_rank"]):
        r_ms, g_ms = pr["render_ms"], pr["gather_ms"]
        assert 0 < r_ms["min"] <= r_ms["mean"] <= r_ms["max"] and r_ms["imbalance"] >= 1.0
        assert 0 <= g_ms["min"] <= g_ms["mean"] <= g_ms["max"] and pr["gather_path"]
