"""Generate the evaluation-metric fixtures by RUNNING the reference's own ``mini_gym_learn/eval_metrics`` modules.

IN-CONTAINER ONLY, like ``make_golden.py`` (whose stubs this uses): nothing here runs on the GPU box, and no
reference source is copied.

Fixtures written:
  eval_metrics.npz   the outputs of every ``METRICS_FNS`` entry on a namespace env of 7 envs with seeded random
                     tensors (planar speed >= 0.1 m/s, so CoT is finite): ``in_*`` the env's tensors, ``h_*`` the outputs
                     with ``measured_heights`` [7, 187], ``s_*`` with the scalar 0 (an env without a height scan);
                     ``zero_in_*`` / ``zero_*``: one more env whose base velocity is exactly zero (CoT = inf or nan);
                     ``names``: the keys of METRICS_FNS in order.  The network metrics run on a stand-in actor-critic
                     (adaptation_module(h) = h @ net_A, env_factor_encoder(p) = tanh(p @ net_B)); auxiliary_rewards on
                     two stand-in reward functions (values aux_r0 / aux_r1, scales 2 and 3), ``h_aux_names`` its keys.
  dr_settings.json   for ``base_set`` and each ``DR_SETTINGS`` entry, every Cfg field the function assigns and its value
                     (found by running it on a Cfg whose leaves were replaced by sentinels, then restored).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval_metrics.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE  # noqa: E402  (installs the stubs and puts the reference on sys.path)

from mini_gym.envs.base.legged_robot_config import Cfg  # noqa: E402
from mini_gym_learn.eval_metrics import domain_randomization as ref_dr  # noqa: E402
from mini_gym_learn.eval_metrics.metrics import METRICS_FNS  # noqa: E402

SEED = 47
N, NH, NHIST, NPRIV, NLAT = 7, 187, 30, 18, 18
NUMERIC = ("lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques",
           "power_consumption", "CoT", "froude_number", "termination")
MASS = 6.921  # default_body_mass of the namespace env


def inputs(rng, n, zero_speed=False):
    f = lambda a: np.asarray(a, np.float32)
    ang = rng.uniform(-np.pi, np.pi, n)
    speed = np.zeros(n) if zero_speed else rng.uniform(0.1, 1.5, n)
    lin = np.stack([speed * np.cos(ang), speed * np.sin(ang), rng.uniform(-0.3, 0.3, n)], 1)
    if zero_speed:
        lin[:] = 0.0
    z = rng.uniform(0.2, 0.45, n)
    root = rng.uniform(-1, 1, (n, 13))
    root[:, 2] = z
    return dict(base_lin_vel=f(lin), base_ang_vel=f(rng.uniform(-1.5, 1.5, (n, 3))),
                commands=f(rng.uniform(-1, 1, (n, 4))), root_states=f(root),
                measured_heights=f(rng.uniform(-0.08, 0.08, (n, NH))), torques=f(rng.uniform(-20, 20, (n, 12))),
                dof_vel=f(rng.uniform(-8, 8, (n, 12))), payloads=f(rng.uniform(-1, 3, n)),
                reset_buf=rng.uniform(0, 1, n) < 0.4)


def namespace_env(inp, heights):
    env = types.SimpleNamespace(**{k: torch.from_numpy(v) for k, v in inp.items()})
    env.default_body_mass = MASS
    if not heights:
        env.measured_heights = 0
    return env


def run(inp, heights, extra=None):
    env = namespace_env(inp, heights)
    out = {}
    for name in NUMERIC:
        out[name] = np.asarray(METRICS_FNS[name](env, None, None))
    if extra is not None:
        ac, obs, r = extra
        env.reward_functions = [lambda: torch.from_numpy(r[0]), lambda: torch.from_numpy(r[1])]
        env.reward_names = ["a", "b"]
        env.reward_scales = {"a": 2.0, "b": 3.0}
        out["adaptation_loss"] = METRICS_FNS["adaptation_loss"](env, ac, obs).numpy()
        out["privileged_obs"] = np.asarray(METRICS_FNS["privileged_obs"](env, ac, obs))
        out["latents"] = np.asarray(METRICS_FNS["latents"](env, ac, obs))
        aux = METRICS_FNS["auxiliary_rewards"](env, ac, obs)
        out["aux_names"] = np.array(list(aux))
        for k, v in aux.items():
            out["auxiliary_rewards_" + k] = v.numpy()
    return out


def gen_metrics():
    rng = np.random.default_rng(SEED)
    inp, zin = inputs(rng, N), inputs(rng, 1, zero_speed=True)
    assert np.all(np.hypot(inp["base_lin_vel"][:, 0], inp["base_lin_vel"][:, 1]) >= 0.1)
    assert inp["reset_buf"].any() and not inp["reset_buf"].all()
    A = (rng.uniform(-1, 1, (NHIST, NLAT)) / np.sqrt(NHIST)).astype(np.float32)
    B = (rng.uniform(-1, 1, (NPRIV, NLAT)) / np.sqrt(NPRIV)).astype(np.float32)
    hist, priv = rng.uniform(-1, 1, (N, NHIST)).astype(np.float32), rng.uniform(-1, 1, (N, NPRIV)).astype(np.float32)
    r = rng.uniform(-1, 1, (2, N)).astype(np.float32)
    ac = types.SimpleNamespace(adaptation_module=lambda h: h @ torch.from_numpy(A),
                               env_factor_encoder=lambda p: torch.tanh(p @ torch.from_numpy(B)))
    obs = {"obs_history": torch.from_numpy(hist), "privileged_obs": torch.from_numpy(priv)}
    save = {"names": np.array(list(METRICS_FNS)), "numeric": np.array(NUMERIC), "default_body_mass": np.float64(MASS),
            "net_A": A, "net_B": B, "obs_history": hist, "privileged_obs_in": priv, "aux_r0": r[0], "aux_r1": r[1]}
    save.update({"in_" + k: v for k, v in inp.items()})
    save.update({"zero_in_" + k: v for k, v in zin.items()})
    save.update({"h_" + k: v for k, v in run(inp, True, (ac, obs, r)).items()})
    save.update({"s_" + k: v for k, v in run(inp, False).items()})
    save.update({"zero_" + k: v for k, v in run(zin, True).items()})
    assert not np.isfinite(save["zero_CoT"]).any() and np.isfinite(save["h_CoT"]).all()
    np.savez(os.path.join(HERE, "eval_metrics.npz"), **save)
    print("eval_metrics.npz:", len(save), "arrays; METRICS_FNS =", list(METRICS_FNS))


class _Sentinel:
    pass


def _leaves(node, path=""):
    for k, v in list(vars(node).items()):
        if k.startswith("_"):
            continue
        p = f"{path}.{k}" if path else k
        if isinstance(v, type):
            yield from _leaves(v, p)
        else:
            yield node, k, p


def assigned_fields(fn):
    """Every Cfg field ``fn`` assigns, {dotted path: value}: the leaves that are no sentinel afterwards (new fields
    included); Cfg is restored."""
    before = [(node, k, getattr(node, k)) for node, k, _ in _leaves(Cfg)]
    known = {(id(node), k) for node, k, _ in before}
    for node, k, _ in before:
        setattr(node, k, _Sentinel())
    try:
        fn()
        out = {p: getattr(node, k) for node, k, p in _leaves(Cfg) if not isinstance(getattr(node, k), _Sentinel)}
        for node, k, _ in list(_leaves(Cfg)):
            if (id(node), k) not in known:
                delattr(node, k)
    finally:
        for node, k, v in before:
            setattr(node, k, v)
    return out


def gen_dr():
    out = {"base_set": assigned_fields(ref_dr.base_set)}
    for name, fn in ref_dr.DR_SETTINGS.items():
        out[name] = assigned_fields(fn)
    with open(os.path.join(HERE, "dr_settings.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("dr_settings.json:", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    gen_metrics()
    gen_dr()
