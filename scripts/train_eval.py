"""Train from scratch, then play — an end-to-end check of the whole stack on one MI355X.

Mini Cheetah, 4096 envs, the upstream semantics the reference's published run had (legacy_fork=False: time-outs
and terminations reset inside step, commands resampled from the grid-adaptive curriculum every 10 s and at
resets); ``--iterations`` PPO iterations of the reference's Runner (24 steps x 4096 envs, 5 epochs x 4
minibatches, the adaptation module trained alongside); then the learned student policy (act_inference:
adaptation module on the history + actor) tracks constant forward commands (scripts/play.py).  Prints one JSON
line: wall time, iterations/s, the tracking rewards early vs late, the command area the curriculum reached, and
the measured forward velocity per command.

  python scripts/train_eval.py [--iterations 1500] [--out DIR] [--terrain-tgs] [--eval-envs N [--eval-set PATH=VALUE ...]]

--terrain-tgs sets Cfg.sim.physx.terrain_solver_type = 1 (TGS on a terrain mesh; the Mini Cheetah preset's plane is
not affected by it).  --eval-envs N adds an eval group of N envs whose cfg is a copy of the train cfg with every
--eval-set PATH=VALUE applied (as scripts/train.py); its episode means are printed as eval_* beside the train ones.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrl import config as lcfg  # noqa: E402
from lrl.env import LeggedRobotEnv  # noqa: E402
from lrl.history import HistoryWrapper  # noqa: E402
from lrl.ppo import runner as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--terrain-tgs", action="store_true",
                    help="on a terrain mesh follow Cfg.sim.physx.solver_type (TGS in the presets) instead of PGS")
    ap.add_argument("--eval-envs", type=int, default=0, help="envs of an eval group after the train envs (0: none)")
    ap.add_argument("--eval-set", action="append", default=[], metavar="PATH=VALUE",
                    help="set a field of the eval cfg (a copy of the train cfg); repeatable")
    a = ap.parse_args()
    if a.eval_set and not a.eval_envs:
        ap.error("--eval-set needs --eval-envs")
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = a.envs
    if a.terrain_tgs:
        cfg.sim.physx.terrain_solver_type = 1
    R.RunnerArgs.save_interval = 0
    R.RunnerArgs.log_freq = 50
    eval_cfg = lcfg.eval_variant(cfg, a.eval_envs, a.eval_set) if a.eval_envs else None
    env = HistoryWrapper(LeggedRobotEnv("cuda:0", cfg=cfg, eval_cfg=eval_cfg, seed=11, legacy_fork=False))
    runner = R.Runner(env, device="cuda:0", seed=11)
    t0 = time.time()
    chunk, hist = 50, []
    done = 0
    while done < a.iterations:
        k = min(chunk, a.iterations - done)
        runner.learn(k, init_at_random_ep_len=(done == 0))
        done += k
        ep = env.env.extras.get("train/episode", {})
        row = {"it": done, "t": round(time.time() - t0, 1)}
        for key in ("rew_total", "rew_tracking_lin_vel", "rew_tracking_ang_vel", "command_area"):
            v = ep.get(key)
            if v is not None:
                row[key] = round(float(v), 5)
        for key, v in env.env.extras.get("eval/episode", {}).items() if eval_cfg is not None else ():
            if key in ("rew_total", "rew_tracking_lin_vel", "rew_tracking_ang_vel"):
                row["eval_" + key] = round(float(v), 5)
        hist.append(row)
        print(json.dumps(row), flush=True)
    wall = time.time() - t0
    sd = runner.alg.actor_critic.state_dict()
    out = a.out or os.path.join(ROOT, "gpurun_out", "train_eval")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "ac_weights_last.pt")
    torch.save({k: v.detach().cpu() for k, v in sd.items()}, path)
    env.env.close()
    import play
    evals = {}
    for vx in (0.0, 0.5, 1.0):
        vel, upright, _ = play.play("mc", path, num_envs=64, steps=500, vx=vx)
        evals[str(vx)] = {"measured_vx": round(float(vel[250:, :, 0].mean()), 4), "upright": upright}
    print(json.dumps({"iterations": a.iterations, "wall_s": round(wall, 1),
                      "iterations_per_s": round(a.iterations / wall, 3),
                      "env_steps_per_s": round(a.iterations * a.envs * 24 / wall, 1),
                      "first": hist[0], "last": hist[-1], "play": evals}), flush=True)


if __name__ == "__main__":
    main()
