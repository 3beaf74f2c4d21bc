"""A few steps of the navigation wrapper for a kernel trace: which launches one ``HighLevelControlWrapper.step`` makes.

Builds the wrapper of scripts/high_level_train.py (Go1, 1,024 envs, the low-level student policy from a checkpoint),
runs ``--warmup`` steps and then ``--steps`` steps with random commands, and prints one JSON line with the host time per
step (device-synchronised around the timed steps).  Run it under ``rocprofv3 --kernel-trace --stats`` and divide each
kernel's calls by ``warmup + steps + 1`` (the constructor's reset makes one zero-action low-level step):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python scripts/nav_step_trace.py tests/golden/checkpoint_last.npz --native 1

usage: python scripts/nav_step_trace.py LOW_LEVEL_CHECKPOINT [--native 0|1] [--num-envs N] [--steps K] [--warmup W]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("low_level")
    ap.add_argument("--native", type=int, default=1, choices=[0, 1])
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import torch
    from high_level_train import load_low_level
    from lrl.high_level import HighLevelControlWrapper

    env = HighLevelControlWrapper.from_actor_critic(load_low_level(a.low_level), num_envs=a.num_envs, device="cuda:0",
                                                    native=bool(a.native))
    env.reset()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    acts = torch.rand(a.warmup + a.steps, a.num_envs, 3, device="cuda:0", generator=gen) * 4 - 2
    with torch.inference_mode():
        for t in range(a.warmup):
            env.step(acts[t])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(a.warmup, a.warmup + a.steps):
            env.step(acts[t])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(json.dumps(dict(native=bool(a.native), num_envs=a.num_envs, steps=a.steps, warmup=a.warmup,
                          ms_per_step=round(1e3 * dt / a.steps, 4))))
    env.ll_env.env.close()
