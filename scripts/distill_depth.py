"""Distil the height scan from the depth camera: train a ``DepthEncoder`` (lrl/vision.py) to predict the scan columns of
``obs`` from the egocentric depth image and the proprioceptive columns, on the rollouts of a trained policy.

The env is the Go1 rough-terrain env of bench.py's ``secondary`` line (curriculum trimesh, upstream resets) with the
height scan on (``terrain.measure_heights``, 187 columns at the end of ``obs``) and the depth camera of
``lrl.config.add_depth_camera``.  The checkpoint's student policy (adaptation module + actor, ``act_student_fused``)
drives it.  After every step that redrew all images (``env.depth_refreshed``) the distiller collects the training envs'
(image, extra, target) rows; the last tenth of the envs is held out: their rows are never collected, and the loss on
their current images is logged beside the training loss.  Each iteration is ``--steps`` env steps and ``--updates`` Adam
steps.  One JSON line per iteration on stdout (and in ``--log``); the encoder's state dict goes to
``depth_encoder_last.pt`` in ``--out-dir``.

``--train-iterations K``: when CKPT does not exist, first train a policy on the same env for K PPO iterations and save its
state dict there (a way to get a checkpoint to try the script on; a real run hands over a trained one).

  python scripts/distill_depth.py CKPT [--iterations 50] [--envs 4096] [--steps 25] [--updates 20] [--out-dir .]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

import torch  # noqa: E402

from lrl import config as lcfg  # noqa: E402
from lrl import vision  # noqa: E402
from lrl.env import LeggedRobotEnv  # noqa: E402
from lrl.history import HistoryWrapper  # noqa: E402
from lrl.ppo.actor_critic import ActorCritic  # noqa: E402


def make_env(num_envs, device, seed=4321, depth=True, sensor=False):
    """bench.py's bench_go1_rough env with the height scan on, and the depth camera (``sensor``: and its sensor
    model, lrl.config.add_depth_sensor's defaults)"""
    cfg = lcfg.make_cfg()
    lcfg.config_go1(cfg)
    cfg.env.num_envs = num_envs
    cfg.terrain.mesh_type = "trimesh"
    cfg.terrain.terrain_proportions = [0.1, 0.1, 0.35, 0.25, 0.2]
    cfg.terrain.curriculum = True
    cfg.terrain.measure_heights = True
    cfg.env.num_observations = 42 + len(cfg.terrain.measured_points_x) * len(cfg.terrain.measured_points_y)
    if depth:
        lcfg.add_depth_camera(cfg)
        if sensor:
            lcfg.add_depth_sensor(cfg)
    return HistoryWrapper(LeggedRobotEnv(device, cfg=cfg, seed=seed, legacy_fork=False)), cfg


def train_policy(path, num_envs, iterations, device):
    from lrl.ppo import runner as R
    env, _ = make_env(num_envs, device, depth=False)
    runner = R.Runner(env, device=device, seed=4321, logger=R.Logger())
    runner.learn(iterations, init_at_random_ep_len=True)
    torch.save({k: v.detach().cpu() for k, v in runner.alg.actor_critic.state_dict().items()}, path)
    env.env.close()


def distill(ckpt, iterations=50, num_envs=4096, steps=25, updates=20, out_dir=".", log=None, device="cuda:0",
            capacity=None, batch_size=1024, lr=1e-3, sensor=False):
    """``sensor``: distil from ``env.depth_sensed`` (noise, holes, quantisation, latency) instead of the exact images."""
    env, cfg = make_env(num_envs, device, sensor=sensor)
    e = env.env
    ac = ActorCritic(cfg.env.num_observations, cfg.env.num_privileged_obs,
                     cfg.env.num_observations * cfg.env.num_observation_history, cfg.env.num_actions)
    ac.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True), strict=True)
    ac = ac.to(device)
    first, scan = vision.scan_columns(e)
    h, w = e.depth_images.shape[1:]
    enc = vision.DepthEncoder(h, w, scan, extra_dim=first, hidden=128, far=float(cfg.depth.far)).to(device)
    n_train = num_envs - max(num_envs // 10, 1)
    train_ids = torch.arange(n_train, device=device)
    d = vision.DepthDistiller(e, enc, capacity=capacity or 4 * n_train, batch_size=batch_size, lr=lr,
                              sensed=sensor)
    obs = env.reset()
    lines = []
    t0 = time.perf_counter()
    for it in range(iterations):
        held = []
        for _ in range(steps):
            with torch.no_grad():
                actions = ac.act_student_fused(obs["obs"].contiguous(), obs["obs_history"])[0]
            obs, _, _, _ = env.step(actions)
            if e.depth_refreshed:
                d.collect(obs["obs"], train_ids)
                img = e.depth_sensed if sensor else e.depth_images
                held.append(d.evaluate(img[n_train:].contiguous(), obs["obs"][n_train:]))
        train_loss = d.update(updates)
        line = {"iteration": it, "rows": d.size, "train_loss": round(float(train_loss), 6),
                "held_out_loss": round(float(torch.stack(held).mean()), 6) if held else None,
                "seconds": round(time.perf_counter() - t0, 2), "native": d.native}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if log:
            with open(log, "a") as f:
                f.write(json.dumps(line) + "\n")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "depth_encoder_last.pt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in enc.state_dict().items()},
                "height": h, "width": w, "out_dim": scan, "extra_dim": first, "hidden": 128, "far": enc.far}, path)
    e.close()
    return path, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ckpt")
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=25, help="env steps per iteration")
    ap.add_argument("--updates", type=int, default=20, help="Adam steps per iteration")
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file")
    ap.add_argument("--train-iterations", type=int, default=0)
    ap.add_argument("--sensor", action="store_true", help="distil from the sensor model's images (env.depth_sensed)")
    a = ap.parse_args()
    if not os.path.exists(a.ckpt):
        if a.train_iterations <= 0:
            sys.exit(f"{a.ckpt} does not exist (--train-iterations K trains a policy to try the script on)")
        train_policy(a.ckpt, a.envs, a.train_iterations, "cuda:0")
    path, lines = distill(a.ckpt, a.iterations, a.envs, a.steps, a.updates, a.out_dir, a.log,
                          sensor=a.sensor)
    print(json.dumps({"saved": path, "first_held_out_loss": lines[0]["held_out_loss"],
                      "last_held_out_loss": lines[-1]["held_out_loss"]}))


if __name__ == "__main__":
    main()
