"""Cost of the egocentric depth camera (lrl_sim_depth: the rigid-body refresh + depth_kernel) per call, next to the env
step it runs beside.

For the Mini Cheetah plane env and the Go1 rough-terrain env of bench.py --full's ``secondary`` (4096 envs each, the
default camera of lrl.config.add_depth_camera): after a few random-action steps, HIP events around ``--calls`` calls
after ``--warmup`` warm-ups, for a full refresh and for ``only_reset`` with no reset flag set; the env step kernel's
own time (lrl_sim_timing) and the whole step's stream time over the same job's steps; and the sha256 of the depth and
id images of one full refresh, so that two builds of the library (LRL_LIB=...) can be compared for bit-identical
images.  One JSON line per env.

  python scripts/depth_timing.py [--envs 4096] [--calls 100] [--warmup 10] [--label cur] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

import torch  # noqa: E402

from lrl import _abi  # noqa: E402
from lrl import config as lcfg  # noqa: E402
from lrl.env import LeggedRobotEnv  # noqa: E402


def make_cfg(kind, n):
    cfg = lcfg.make_cfg()
    if kind == "mc_plane":
        lcfg.config_mini_cheetah(cfg)
    else:  # bench.py's bench_go1_rough
        lcfg.config_go1(cfg)
        cfg.terrain.mesh_type = "trimesh"
        cfg.terrain.terrain_proportions = [0.1, 0.1, 0.35, 0.25, 0.2]
        cfg.terrain.curriculum = True
    cfg.env.num_envs = n
    lcfg.add_depth_camera(cfg)
    return cfg


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def measure(kind, n, calls, warmup, steps, dev):
    env = LeggedRobotEnv(dev, cfg=make_cfg(kind, n), seed=4321)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(1)
    acts = [torch.rand(n, 12, device=dev, generator=gen) * 2 - 1 for _ in range(steps)]
    cam, env._depth_cam = env._depth_cam, None  # (the steps below are timed without the sensor's launches)
    for a in acts[:warmup]:
        env.step(a)
    env.kernel_timing(True)
    it = iter(acts[warmup:])
    step_ms = events_ms(lambda: env.step(next(it)), steps - warmup)
    kernel_ms = env.kernel_timing(False)[0]
    env._depth_cam = cam
    depth = env.depth_images
    ids = torch.empty(depth.shape, dtype=torch.int32, device=dev)
    L, st = _abi.lib(), env._stream()

    def call(only_reset, with_ids=False):
        _abi.check(L.lrl_sim_depth(env._sim, C.byref(cam), 0, n, only_reset, C.c_void_p(depth.data_ptr()),
                                   C.c_void_p(ids.data_ptr()) if with_ids else None, st))
    call(0, True)
    torch.cuda.synchronize()
    sha = hashlib.sha256(depth.cpu().numpy().tobytes() + ids.cpu().numpy().tobytes()).hexdigest()[:16]
    hit = float((ids > 0).float().mean())
    robot = float((ids > 1).float().mean())
    out = {"env": kind, "envs": n, "width": cam.width, "height": cam.height, "rays": n * cam.width * cam.height,
           "calls": calls, "warmup": warmup}
    env._reset_u8.zero_()
    for key, only_reset in (("full_refresh_ms", 0), ("only_reset_no_flags_ms", 1)):
        for _ in range(warmup):
            call(only_reset)
        out[key] = round(events_ms(lambda: call(only_reset), calls), 4)
    refresh_ms = events_ms(env.refresh_rigid_body_state, calls)
    out.update(rigid_body_refresh_ms=round(refresh_ms, 4), env_step_kernel_ms=round(kernel_ms, 4),
               env_step_stream_ms=round(step_ms, 4), steps_timed=steps - warmup,
               amortised_ms_per_step_interval_5=round((out["full_refresh_ms"] + 4 * out["only_reset_no_flags_ms"]) / 5, 4),
               pixels_hit_fraction=round(hit, 4), pixels_on_robot_fraction=round(robot, 4), images_sha256=sha)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=60, help="env steps before the measurement (the last 50 are timed)")
    ap.add_argument("--kinds", default="mc_plane,go1_rough")
    ap.add_argument("--label", default="cur")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for kind in a.kinds.split(","):
        r = dict(label=a.label, **measure(kind, a.envs, a.calls, a.warmup, a.steps, "cuda:0"))
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
