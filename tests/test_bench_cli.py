"""bench.py's multi-rank launch: ``--gpus N`` starts N ranks itself, every rank joins one
process group of exactly N ranks, and asking for more GPUs than are visible fails instead of running a
mislabelled single-rank job.  On a GPU: a plain run's result line and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    r = _run(["--gpus", str(n), "--world-check"], LRL_DIST_BACKEND="gloo")
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout  # rank 0 alone prints
    out = json.loads(line[0])
    assert out["world_size"] == n and out["ranks"] == list(range(n)) and out["parallelism"] == f"dp{n}"


def test_more_gpus_than_visible_fails():
    import torch
    n = torch.cuda.device_count() + 1
    r = _run(["--gpus", str(n), "--world-check"], LRL_DIST_BACKEND="nccl")
    assert r.returncode != 0
    assert "GPU(s) visible" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    """A plain run times exactly --steps iterations and reports the headline alone (the other figures are --full's);
    --dump-outputs writes the last iteration's arrays as float32 .npy files, 64 MB at the most."""
    import numpy as np
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    assert out["steps"] == 1 and out["warmup"] == 1 and out["unit"] == "env-steps/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(4096 * 24 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert not {"secondary", "cpu_baseline", "roofline", "self_contact", "env_step_kernel_ms"} & set(out)
    files = sorted(os.listdir(tmp_path / "out"))
    arrays = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert {"policy.std", "rollout.actions", "rollout.returns", "env.obs", "env.obs_history"} <= set(arrays)
    assert arrays["rollout.actions"].shape == (24, 4096, 12) and arrays["env.obs"].shape == (4096, 42)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--world-check"], LRL_DIST_BACKEND="gloo", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
