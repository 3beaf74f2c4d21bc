"""Cost of the depth sensor model (lrl_sim_depth_sense, Cfg.depth_sensor) per depth tick, next to the tick without it.

The Mini Cheetah plane env at 4096 envs with the default camera (64 x 48) and the default sensor model at
``latency_frames`` [0, 0] and [0, 1]: HIP events around ``--calls`` calls of the env's depth tick (the exact image's
launches, then the sensor's) after ``--warmup`` warm-ups, for a full refresh (the sensor pushes a frame) and for an
off-interval tick with no reset flag set (both launches' workgroups return at once).  Blocks with the sensor's launch
and without it alternate ``--blocks`` times inside the one process; every block's figure is kept.  One JSON line per
case.

  python scripts/depth_sensor_timing.py [--envs 4096] [--calls 200] [--warmup 20] [--blocks 3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

import torch  # noqa: E402

from lrl import config as lcfg  # noqa: E402
from lrl.env import LeggedRobotEnv  # noqa: E402


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def measure(n, latency, calls, warmup, blocks, dev):
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = n
    lcfg.add_depth_camera(cfg)
    lcfg.add_depth_sensor(cfg, latency_frames=latency)
    env = LeggedRobotEnv(dev, cfg=cfg, seed=4321)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(1)
    for _ in range(10):
        env.step(torch.rand(n, 12, device=dev, generator=gen) * 2 - 1)
    env._reset_u8.zero_()
    sensor, interval = env._depth_sensor, env._depth_interval
    out = {"envs": n, "width": sensor.width, "height": sensor.height, "latency_frames": list(latency),
           "calls": calls, "warmup": warmup, "blocks": blocks,
           "image_mbytes": round(n * sensor.width * sensor.height * 4 / 1e6, 2)}

    def tick(step):
        env._depth_step = step  # a multiple of the interval: a full refresh (push); else reset-only
        env._depth_tick()
    for key, step in (("push", 7 * interval), ("reset_only_no_flags", 7 * interval + 1)):
        on, off = [], []
        for _ in range(blocks):
            for with_sensor, dst in ((False, off), (True, on)):
                env._depth_sensor = sensor if with_sensor else None
                for _ in range(warmup):
                    tick(step)
                dst.append(round(events_ms(lambda: tick(step), calls), 4))
        env._depth_sensor = sensor
        out[key + "_tick_ms_sensor_off"] = off
        out[key + "_tick_ms_sensor_on"] = on
        out[key + "_sensor_ms"] = round(statistics.median(on) - statistics.median(off), 4)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--label", default="cur")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for latency in ([0, 0], [0, 1]):
        line = json.dumps(dict(label=a.label, **measure(a.envs, latency, a.calls, a.warmup, a.blocks, "cuda:0")))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
