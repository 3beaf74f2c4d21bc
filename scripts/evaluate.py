"""Evaluate a trained policy under the reference's evaluation presets, with the metrics accumulated on the device.

For each ``--preset`` (default: all six of ``lrl.config.DR_PRESETS``) a stand-alone env is built from the robot preset +
``base_set`` + the preset (``lrl.config.eval_variant``: 500 s episodes, termination on body height 0, no command
resampling, 10 x 10 tiles), the student policy (act_inference: adaptation module on the history + actor, as
scripts/play.py) tracks the constant command ``--vx / --vy / --wz`` for ``--steps`` policy steps after 20 zero-action
steps, and one JSON line of ``EvalMetrics.summary("all")`` is printed: mean / std / max of every metric over the
env-steps, the true velocity RMSD, the cost of transport, and the episode / fall / step counts.  No per-step host copy.

  python scripts/evaluate.py CHECKPOINT [--robot mc|go1] [--envs 64] [--steps 1000] [--preset NAME ...] [--vx 1.0]

CHECKPOINT: an ActorCritic state dict (a run's checkpoints/ac_weights_last.pt), loaded with ``weights_only=True``.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from lrl import config as lcfg  # noqa: E402
from lrl.env import LeggedRobotEnv  # noqa: E402
from lrl.eval_metrics import EvalMetrics  # noqa: E402
from lrl.history import HistoryWrapper  # noqa: E402


def evaluate(checkpoint, robot="mc", preset="static_medium", num_envs=64, steps=1000, vx=1.0, vy=0.0, wz=0.0,
             device="cuda:0", seed=0):
    """One preset's ``summary("all")`` (plus what was run)."""
    from play import load_policy
    base = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(base)
    cfg = lcfg.eval_variant(base, num_envs, preset=("base_set", preset))
    env = HistoryWrapper(LeggedRobotEnv(device, cfg=cfg, seed=seed))
    e = env.env
    try:
        policy = load_policy(checkpoint, cfg, device)
        metrics = EvalMetrics(e)

        def command():
            e.commands[:, 0], e.commands[:, 1], e.commands[:, 2] = vx, vy, wz

        command()
        obs = env.reset()
        actions = torch.zeros(num_envs, 12, device=device)
        with torch.no_grad():
            for _ in range(20):  # settle, as play_mc does; not measured
                command()
                obs, _, _, _ = env.step(actions)
            metrics.enable()
            metrics.clear()
            for _ in range(steps):
                actions = policy(obs)
                command()
                obs, _, _, _ = env.step(actions)
        out = metrics.summary("all")
    finally:
        e.close()
    return dict({"preset": preset, "robot": robot, "envs": num_envs, "command": [vx, vy, wz]}, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--robot", default="mc", choices=["mc", "go1"])
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--preset", action="append", default=None, choices=list(lcfg.DR_PRESETS), metavar="NAME",
                    help="an evaluation preset (%s); repeatable, default: all" % ", ".join(lcfg.DR_PRESETS))
    ap.add_argument("--vx", type=float, default=1.0)
    ap.add_argument("--vy", type=float, default=0.0)
    ap.add_argument("--wz", type=float, default=0.0)
    a = ap.parse_args()
    for preset in a.preset or lcfg.DR_PRESETS:
        row = evaluate(a.checkpoint, a.robot, preset, a.envs, a.steps, a.vx, a.vy, a.wz)
        # strict JSON: a non-finite value (the CoT maximum of an env that stood still) becomes null
        row = {k: None if isinstance(v, float) and not math.isfinite(v) else v for k, v in row.items()}
        print(json.dumps(row, allow_nan=False), flush=True)


if __name__ == "__main__":
    main()
