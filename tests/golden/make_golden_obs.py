"""Generate the observation-layout fixtures by RUNNING the reference's own ``LeggedRobot.step``.

IN-CONTAINER ONLY, like ``make_golden.py`` (whose stubs, fake simulator and ``gen_post_physics`` this imports):
nothing here runs on the GPU box, and no reference source is copied.

Fixtures written (16 envs x 3 steps each, the format of post_physics_*.npz):
  post_physics_obs_lin.npz         Mini Cheetah, env.observe_only_lin_vel, noise on                       45 obs
  post_physics_obs_ang.npz         Mini Cheetah, env.observe_only_ang_vel, add_noise off (with noise the
                                   reference raises: its noise vector has no entries for the block)      45 obs
  post_physics_obs_yaw_global.npz  Go1, observe_vel + observe_yaw + commands.global_reference, noise on  49 obs
  post_physics_obs_all.npz         Go1, all five switches, add_noise off                                 55 obs

``make_golden.rand_quat`` tilts by at most 0.6 rad, which would leave the yaw entry (0.5 x heading, clipped to
[-1, 1]) unclipped everywhere, so the yaw cases draw their orientations from ``yaw_rand_quat``: a uniform yaw in
(-pi, pi) composed with that tilt.  The script asserts that every heading keeps 1e-3 rad from the +-pi wrap and that
unclipped, clipped-high and clipped-low headings all occur.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_obs.py
"""
import os

import numpy as np

import make_golden
from make_golden import HERE, gen_post_physics

SEED = 31
CASES = {
    "lin": ("mc", {"env.observe_only_lin_vel": True, "env.num_observations": 45}),
    "ang": ("mc", {"env.observe_only_ang_vel": True, "noise.add_noise": False, "env.num_observations": 45}),
    "yaw_global": ("go1", {"env.observe_vel": True, "env.observe_yaw": True, "commands.global_reference": True,
                           "env.num_observations": 49}),
    "all": ("go1", {"env.observe_vel": True, "env.observe_only_ang_vel": True, "env.observe_only_lin_vel": True,
                    "env.observe_yaw": True, "commands.global_reference": True, "noise.add_noise": False,
                    "env.num_observations": 55}),
}

_tilt_quat = make_golden.rand_quat


def yaw_rand_quat(rng, n, tilt=0.6):
    """q_yaw * q_tilt (xyzw): make_golden.rand_quat's tilt, then a uniform yaw about the world z axis."""
    t = _tilt_quat(rng, n, tilt).astype(np.float64)
    yaw = rng.uniform(-np.pi, np.pi, n)
    z, w = np.sin(yaw / 2), np.cos(yaw / 2)
    x2, y2, z2, w2 = t.T
    q = np.stack([w * x2 - z * y2, w * y2 + z * x2, w * z2 + z * w2, w * w2 - z * z2], axis=1)
    return q.astype(np.float32)


def heading(quat):
    """atan2 of the rotated x axis (legged_robot.py:379-380) in float64."""
    x, y, z, w = np.asarray(quat, np.float64).T
    return np.arctan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))


def tweak_of(over):
    def tweak(cfg):
        for k, v in over.items():
            node = cfg
            *ps, leaf = k.split(".")
            for p in ps:
                node = getattr(node, p)
            assert hasattr(node, leaf), k
            setattr(node, leaf, v)
    return tweak


def gen(case):
    robot, over = CASES[case]
    name = f"post_physics_obs_{case}.npz"
    yaw = bool(over.get("env.observe_yaw"))
    make_golden.rand_quat = yaw_rand_quat if yaw else _tilt_quat
    try:
        gen_post_physics(robot, tweak=tweak_of(over), seed=SEED, name=name)
    finally:
        make_golden.rand_quat = _tilt_quat
    g = np.load(os.path.join(HERE, name))
    assert g["obs"].shape == (3, 16, over["env.num_observations"]), g["obs"].shape
    if yaw:
        h = heading(g["root_in"][..., 3:7].reshape(-1, 4))
        assert np.all(np.pi - np.abs(h) > 1e-3), "a heading sits on the +-pi wrap: pick another seed"
        classes = [int(np.sum(np.abs(h) <= 2.0)), int(np.sum(h > 2.0)), int(np.sum(h < -2.0))]
        assert min(classes) > 0, f"heading classes (unclipped, high, low) {classes}: pick another seed"
        col = g["obs"].shape[2] - 1
        print(case, "headings unclipped / clipped high / clipped low:", classes, "wrap margin",
              float(np.min(np.pi - np.abs(h))), "yaw column", float(g["obs"][..., col].min()),
              float(g["obs"][..., col].max()))
    if over.get("commands.global_reference"):
        d = np.abs(g["root_in"][..., 7:10] - g["base_lin_vel"]).max()
        print(case, "max |world - body linear velocity|", float(d))


def check_refused():
    """observe_only_ang_vel with noise: the reference's own step raises (45 obs against a 42-entry noise vector)."""
    over = dict(CASES["ang"][1], **{"noise.add_noise": True})
    try:
        gen_post_physics("mc", tweak=tweak_of(over), seed=SEED, name="_refused.npz")
    except RuntimeError as e:
        print("observe_only_ang_vel + add_noise raises RuntimeError:", e)
        return
    raise AssertionError("the reference ran observe_only_ang_vel with noise")


if __name__ == "__main__":
    for c in CASES:
        gen(c)
    check_refused()
