"""The evaluation-metrics kernels on the device (csrc/lrl_metrics.hip through lrl.eval_metrics.EvalMetrics): the per-step
table and the per-env totals against the float64 checker tests/metrics_ref.py evaluated over the env's own public
tensors, the counters, the group reduction, "off means off", the Runner's logging and scripts/evaluate.py.

n = 70 envs (64 + a tail of 6, rows padded to 128: lanes e >= n exist); 45 train + 25 eval envs where a group split is
needed, so the boundary falls inside a wave."""
import copy
import ctypes as C
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref
from helpers import make_rough, same
from lrl import _abi
from lrl import config as lcfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_TRAIN, N_EVAL = 70, 45, 25
SENTINEL = -777.0


def _np(t):
    return t.detach().cpu().numpy()


def _cfg(robot, n, **over):
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    cfg.env.num_envs = n
    cfg.env.record_video = False
    lcfg._apply(cfg, over)
    return cfg


def _actions(seed, steps, n):
    g = torch.Generator().manual_seed(seed)
    return (0.6 * torch.randn(steps, n, 12, generator=g)).to("cuda:0")


def _public(env):
    """The checker's inputs: the env's own public tensors, as numpy."""
    h = env.measured_heights
    return dict(base_lin_vel=_np(env.base_lin_vel), base_ang_vel=_np(env.base_ang_vel), commands=_np(env.commands),
                torques=_np(env.torques), dof_vel=_np(env.dof_vel), root_states=_np(env.root_states),
                payloads=_np(env.payloads), reset_buf=_np(env.reset_buf), default_body_mass=env.default_body_mass,
                measured_heights=_np(h) if torch.is_tensor(h) else h)


def _step_rows(m):
    step = _np(m.tables()["step"])
    return {k: step[i] for i, k in enumerate(metrics_ref.ROWS)}


def _fill_sentinel(m):
    """Every element of every table, pad lanes included; the clear that follows rewrites the lanes e < n only."""
    for k, t in m.tables(padded=True).items():
        t.fill_(SENTINEL)
    m.clear()


def _assert_pad_untouched(m, n):
    for k, t in m.tables(padded=True).items():
        pad = _np(t[..., n:])
        assert pad.size > 0 and np.all(pad == SENTINEL), f"{k}: a lane e >= n was written"


def _run_and_check(env, steps, seed):
    """`steps` physics steps with seeded random actions: after each one the step table against the checker, at the end
    the totals against the checker's float64 running sums of the table's own float32 values."""
    from lrl.eval_metrics import EvalMetrics
    n = env.num_envs
    env.reset()
    m = EvalMetrics(env).enable()
    assert m.pitch == 128 and m.rows == _abi.METRIC_ROWS
    _fill_sentinel(m)
    tot = metrics_ref.Totals(n)
    worst = {}
    # commands that differ from env to env (the fork's steps do not resample them): the tracking errors are no copies
    env.commands[:, :3] = (2 * torch.rand(n, 3, generator=torch.Generator().manual_seed(seed + 100)) - 1).to("cuda:0")
    for a in _actions(seed, steps, n):
        env.step(a)
        torch.cuda.synchronize()
        ref = metrics_ref.metrics(**_public(env))
        rows = _step_rows(m)
        for k, v in metrics_ref.check(rows, ref, what=f"step {tot.steps[0]}").items():
            worst[k] = max(worst.get(k, 0.0), v)
        tot.add(rows, _np(env.reset_buf), _np(env.time_out_buf))
    print("largest error / bar per row:", {k: round(v, 4) for k, v in worst.items()})
    _check_totals(m, tot)
    _assert_pad_untouched(m, n)
    return m, tot


def _check_totals(m, tot):
    t = {k: _np(v) for k, v in m.tables().items()}
    for i, k in enumerate(metrics_ref.ROWS):
        if k == "CoT":  # never accumulated
            assert np.all(t["sum"][i] == 0.0) and np.all(t["sumsq"][i] == 0.0)
        else:
            # the same float32 values added in float64 in the same order: only a contraction could differ
            assert np.all(np.abs(t["sum"][i] - tot.sum[k]) <= 1e-12 * tot.abs[k]), k
            assert np.all(np.abs(t["sumsq"][i] - tot.sumsq[k]) <= 1e-12 * tot.sumsq[k]), k
        same(t["max"][i], tot.max[k], f"max of {k}")
    same(t["steps"], tot.steps, "steps")
    same(t["episodes"], tot.episodes, "episodes")
    same(t["falls"], tot.falls, "falls")


# ---- 5. per-step table and totals
@pytest.mark.parametrize("robot", ["go1", "mc"])
def test_step_table_and_totals(robot):
    from lrl.env import LeggedRobotEnv
    env = LeggedRobotEnv("cuda:0", cfg=_cfg(robot, N), seed=3)
    try:
        assert not torch.is_tensor(env.measured_heights)  # base_height is root z here
        m, tot = _run_and_check(env, 8, seed=21 if robot == "go1" else 22)
        assert np.all(tot.steps == 8)
        # per_env() is the same totals as statistics
        pe = {k: _np(v) for k, v in m.per_env().items()}
        assert np.all(np.abs(pe["lin_vel_x/mean"] - tot.sum["lin_vel_x"] / 8) <= 1e-12 * tot.abs["lin_vel_x"] / 8)
        same(pe["max_torques/max"], tot.max["max_torques"], "per_env max")
        mass = (np.float32(env.default_body_mass) + _np(env.payloads)).astype(np.float64)
        weight_dist = mass * 9.8 * tot.sum["speed_xy"]
        want = tot.sum["power_consumption"] / weight_dist
        assert np.all(np.abs(pe["cost_of_transport"] - want)
                      <= 1e-12 * tot.abs["power_consumption"] / weight_dist + 1e-12 * np.abs(want))
    finally:
        env.close()


# ---- 6. heights
def test_base_height_over_the_height_scan():
    from lrl.env import LeggedRobotEnv
    cfg, _, _, _ = make_rough("go1", **{"terrain.num_rows": 3, "terrain.num_cols": 4,
                                        "terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2]})
    cfg.env.num_envs, cfg.env.record_video = N, False
    cfg.terrain.max_init_terrain_level = min(cfg.terrain.max_init_terrain_level, cfg.terrain.num_rows - 1)
    env = LeggedRobotEnv("cuda:0", cfg=cfg, seed=5)
    try:
        assert env._P.terrain_mesh == 1 and tuple(env.measured_heights.shape) == (N, 187)
        _run_and_check(env, 3, seed=23)
        assert np.abs(_np(env.measured_heights)).max() > 0  # the scan saw terrain, not a plane
    finally:
        env.close()


# ---- 7. counters
def test_episode_and_fall_counters():
    from lrl.env import LeggedRobotEnv
    from lrl.eval_metrics import EvalMetrics
    # dt = 0.02: an episode of 0.08 s times out when its length passes 4 steps
    env = LeggedRobotEnv("cuda:0", cfg=_cfg("go1", N, **{"env.episode_length_s": 0.08}), seed=7, legacy_fork=False)
    try:
        env.reset()
        on_back = torch.tensor([3, 17, 40, 63, 64, 66, 69], device="cuda:0")
        root = env.root_states.clone().contiguous()
        root[on_back, 2] = 0.05  # the base on the ground, upside down: its contact terminates the episode
        root[on_back, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda:0")
        root[on_back, 7:13] = 0.0
        env.set_actor_root_state_tensor_indexed(root, on_back)
        m = EvalMetrics(env).enable()
        m.clear()
        episodes, falls = np.zeros(N, np.int32), np.zeros(N, np.int32)
        zero = torch.zeros(N, 12, device="cuda:0")
        for _ in range(6):
            env.step(zero)
            torch.cuda.synchronize()
            r, t = _np(env.reset_buf), _np(env.time_out_buf)
            episodes += r
            falls += r & ~t
        tab = {k: _np(v) for k, v in m.tables().items()}
        same(tab["episodes"], episodes, "episodes")
        same(tab["falls"], falls, "falls")
        same(tab["steps"], np.full(N, 6, np.int32), "steps")
        # (a base that bounced off the ground within the step shows no contact at its end: not every one falls)
        assert falls.sum() > 0 and falls.sum() == falls[_np(on_back)].sum(), "no env on its back fell, or another did"
        assert (episodes - falls).sum() > 0, "no env timed out"
        s = m.summary("all")
        assert (s["episodes"], s["falls"], s["steps"]) == (int(episodes.sum()), int(falls.sum()), 6 * N)
        assert s["termination/mean"] == episodes.sum() / (6 * N)
    finally:
        env.close()


# ---- 8. group reduction
def _split_env(seed=9, **kw):
    from lrl.env import LeggedRobotEnv
    cfg = _cfg("go1", N_TRAIN)
    return LeggedRobotEnv("cuda:0", cfg=cfg, eval_cfg=lcfg.eval_variant(cfg, N_EVAL, preset="static_high"), seed=seed, **kw)


def test_group_reduction():
    from lrl.eval_metrics import EvalMetrics
    env = _split_env()
    try:
        assert (env.num_train_envs, env.num_envs) == (N_TRAIN, N)
        env.reset()
        m = EvalMetrics(env).enable()
        m.clear()
        tot = metrics_ref.Totals(N)
        for a in _actions(31, 5, N):
            env.step(a)
            torch.cuda.synchronize()
            tot.add(_step_rows(m), _np(env.reset_buf), _np(env.time_out_buf))
        _check_totals(m, tot)
        t = {k: _np(v) for k, v in m.tables().items()}
        mass = (np.float32(env.default_body_mass) + _np(env.payloads)).astype(np.float64)
        R = _abi.METRIC_ROWS
        for group, sl in (("train", slice(0, N_TRAIN)), ("eval", slice(N_TRAIN, N)), ("all", slice(0, N))):
            r = m.reduce(group).numpy()
            assert r.shape == (_abi.METRICS_REDUCE_DOUBLES,)
            same(m.reduce(group).numpy(), r, f"{group}: a second reduction")
            for i, k in enumerate(metrics_ref.ROWS):
                assert abs(r[3 * i] - t["sum"][i, sl].sum()) <= 1e-12 * tot.abs[k][sl].sum(), (group, k)
                assert abs(r[3 * i + 1] - t["sumsq"][i, sl].sum()) <= 1e-12 * tot.sumsq[k][sl].sum(), (group, k)
                assert r[3 * i + 2] == t["max"][i, sl].max(), (group, k)
            steps, episodes, falls = (int(t[k][sl].sum()) for k in ("steps", "episodes", "falls"))
            assert list(r[3 * R:3 * R + 3]) == [steps, episodes, falls] and steps == 5 * (sl.stop - sl.start)
            wd = (mass[sl] * t["sum"][_abi.METRIC_SPEED_XY, sl]).sum()
            assert abs(r[3 * R + 3] - wd) <= 1e-12 * wd
            # the summary is these numbers as statistics
            s = m.summary(group)
            assert json.dumps(s) == json.dumps(m.summary(group))  # bit-identical from call to call
            assert (s["steps"], s["episodes"], s["falls"]) == (steps, episodes, falls)
            for i, k in enumerate(metrics_ref.NAMES):
                assert s[k + "/max"] == r[3 * i + 2]
                if k == "CoT":
                    assert k + "/mean" not in s and k + "/std" not in s
                    continue
                mean = t["sum"][i, sl].sum() / steps
                assert abs(s[k + "/mean"] - mean) <= 1e-12 * tot.abs[k][sl].sum() / steps, (group, k)
                assert s[k + "/std"] == math.sqrt(max(r[3 * i + 1] / steps - (r[3 * i] / steps) ** 2, 0.0))
            i = metrics_ref.NAMES.index("lin_vel_rmsd")
            rms = math.sqrt(t["sumsq"][i, sl].sum() / steps)
            assert abs(s["lin_vel_rmsd_rms"] - rms) <= 1e-12 * rms
            assert s["lin_vel_rmsd_rms"] >= s["lin_vel_rmsd/mean"]  # root mean square >= mean of the absolute error
            cot = t["sum"][metrics_ref.NAMES.index("power_consumption"), sl].sum() / (9.8 * wd)
            assert abs(s["cost_of_transport"] - cot) <= 1e-11 * abs(cot) + 1e-12 * tot.abs["power_consumption"][sl].sum() / (9.8 * wd)
        L = _abi.lib()
        out = torch.zeros(_abi.METRICS_REDUCE_DOUBLES, dtype=torch.float64, device="cuda:0")
        for first, count in ((-1, 4), (0, N + 1), (N, 1), (3, -1)):  # refused without a launch
            assert L.lrl_sim_metrics_reduce(env._sim, C.c_int32(first), C.c_int32(count), C.c_void_p(out.data_ptr()),
                                            env._stream()) == -1
        _abi.check(L.lrl_sim_metrics_reduce(env._sim, C.c_int32(N), C.c_int32(0), C.c_void_p(out.data_ptr()),
                                            env._stream()))  # an empty range: zeros and max -inf
        e = out.cpu().numpy()
        assert np.all(e[0:3 * R:3] == 0) and np.all(e[1:3 * R:3] == 0) and np.all(e[2:3 * R:3] == -np.inf)
        assert np.all(e[3 * R:] == 0)
    finally:
        env.close()


# ---- 9. off means off
def _rollout(env, acts, metrics):
    from lrl.eval_metrics import EvalMetrics
    env.reset()
    m = EvalMetrics(env).enable() if metrics else None
    out = []
    env.kernel_timing(True)
    for a in acts:
        obs, rew, _, _ = env.step(a)
        out.append((_np(obs).copy(), _np(rew).copy(), _np(env.root_states).copy()))
    _, _, launches = env.kernel_timing(False)
    arena = C.c_int64(0)
    _abi.check(env._L.lrl_debug_sim_arena(env._sim, None, C.byref(arena), None))
    return out, launches, arena.value, m


def test_off_means_off():
    from lrl.env import LeggedRobotEnv
    acts = _actions(41, 4, N)
    L = _abi.lib()
    off = LeggedRobotEnv("cuda:0", cfg=_cfg("go1", N), seed=11)
    on = LeggedRobotEnv("cuda:0", cfg=_cfg("go1", N), seed=11)
    try:
        a, launches_off, arena_off, _ = _rollout(off, acts, False)
        b, launches_on, arena_on, m = _rollout(on, acts, True)
        # never enabled: one timed launch per step as before, no tables, the arena as it was
        assert launches_off == len(acts) == launches_on and arena_off == arena_on
        view = _abi.LrlMetricsView()
        assert L.lrl_sim_metrics_tensors(off._sim, C.byref(view)) == -1
        assert L.lrl_sim_metrics_clear(off._sim, off._stream()) == -1
        # enabling metrics does not change the rollout
        for i, (x, y) in enumerate(zip(a, b)):
            for what, u, v in zip(("obs", "rewards", "root states"), x, y):
                same(u, v, f"step {i} {what}")
        assert np.all(_np(m.tables()["steps"]) == len(acts))
        # after disable() the totals (and the step table) stop changing
        m.disable()
        before = {k: _np(v).copy() for k, v in m.tables().items()}
        for x in acts[:2]:
            on.step(x)
        torch.cuda.synchronize()
        for k, v in m.tables().items():
            same(_np(v), before[k], f"{k} after disable()")
        m.enable()  # and on again: the totals continue
        on.step(acts[0])
        torch.cuda.synchronize()
        assert np.all(_np(m.tables()["steps"]) == len(acts) + 1)
    finally:
        off.close()
        on.close()


def test_metrics_fns_read_the_device_table():
    """mini_gym_learn.eval_metrics.metrics on a native env: the torch form before the first metered step, the table's
    rows afterwards; both are the checker's values."""
    from lrl.env import LeggedRobotEnv
    from mini_gym_learn.eval_metrics.metrics import METRICS_FNS
    env = LeggedRobotEnv("cuda:0", cfg=_cfg("go1", N), seed=13)
    try:
        env.reset()
        for step, a in enumerate(_actions(51, 2, N)):
            if step:
                env.step(a)
            torch.cuda.synchronize()
            ref = metrics_ref.metrics(**_public(env))
            got = {k: METRICS_FNS[k](env, None, None) for k in metrics_ref.NAMES}
            assert all(v.device.type == "cpu" and tuple(v.shape) == (N,) for v in got.values())
            metrics_ref.check({k: v.numpy() for k, v in got.items()}, ref, rows=metrics_ref.NAMES, what=f"call {step}")
            assert env._metrics_fns.enabled
            if step:
                same(got["power_consumption"].numpy(), _step_rows(env._metrics_fns)["power_consumption"], "table row")
    finally:
        env.close()


# ---- 10. Runner and script
def test_runner_logs_eval_metrics():
    from lrl.history import HistoryWrapper
    from lrl.ppo import runner as R

    class Capture(R.Logger):
        def __init__(self):
            super().__init__(None)
            self.seen = {}

        def store_metrics(self, metrics=None, **kw):
            for k, v in dict(metrics or {}, **kw).items():
                self.seen.setdefault(f"{self._metrics_prefix}/{k}" if self._metrics_prefix else k, []).append(v)
            return super().store_metrics(metrics, **kw)

    saved = {k: getattr(R.RunnerArgs, k) for k in ("log_eval_metrics", "save_interval", "save_video_interval")}
    R.RunnerArgs.log_eval_metrics, R.RunnerArgs.save_interval, R.RunnerArgs.save_video_interval = True, 0, 0
    env = HistoryWrapper(_split_env(seed=17))
    try:
        lg = Capture()
        runner = R.Runner(env, device="cuda:0", seed=17, logger=lg)
        assert runner.eval_metrics is not None and R.RunnerArgs.num_steps_per_env == 24
        runner.learn(1, eval_freq=1)
        logged = {k: v for k, v in lg.seen.items() if k.startswith("eval/metrics/")}
        assert logged["eval/metrics/steps"] == [N_EVAL * 24]
        for k in metrics_ref.NAMES:
            if k != "CoT":
                assert math.isfinite(logged[f"eval/metrics/{k}/mean"][0]) and math.isfinite(logged[f"eval/metrics/{k}/std"][0]), k
        for k in ("lin_vel_rmsd_rms", "cost_of_transport", "episodes", "falls", "max_torques/max"):
            assert math.isfinite(logged["eval/metrics/" + k][0]), k
        assert np.all(_np(runner.eval_metrics.tables()["steps"]) == 0)  # cleared for the next batch
    finally:
        for k, v in saved.items():
            setattr(R.RunnerArgs, k, v)
        env.env.close()


def test_runner_default_leaves_metrics_off():
    from lrl.history import HistoryWrapper
    from lrl.ppo import runner as R
    env = HistoryWrapper(_split_env(seed=17))
    try:
        runner = R.Runner(env, device="cuda:0", seed=17, logger=R.Logger(None))
        assert runner.eval_metrics is None
        assert _abi.lib().lrl_sim_metrics_tensors(env.env._sim, C.byref(_abi.LrlMetricsView())) == -1
    finally:
        env.env.close()


def test_evaluate_script_prints_one_json_line(tmp_path):
    """scripts/evaluate.py on the checkpoint the reference's training flow writes (tests/test_train_script_gpu.py)."""
    from ml_logger import logger
    from mini_gym.envs.base.legged_robot_config import Cfg
    from mini_gym_learn.ppo import RunnerArgs
    saved = copy.deepcopy(Cfg)
    saved_args = dict(save_interval=RunnerArgs.save_interval, log_freq=RunnerArgs.log_freq)
    RunnerArgs.save_interval, RunnerArgs.log_freq = 400, 1
    spec = importlib.util.spec_from_file_location("lrl_scripts_train_for_eval", os.path.join(ROOT, "scripts", "train.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    try:
        logger.configure(logger.utcnow("rapid-locomotion/%Y-%m-%d/train/%H%M%S.%f"), root=str(tmp_path))
        runner = script.train_mc(headless=True, iterations=1, robot="go1")
        ckpt = os.path.join(logger.run_dir, "checkpoints", "ac_weights_last.pt")
        runner.env.env.close()
        assert os.path.exists(ckpt)
    finally:
        RunnerArgs.save_interval, RunnerArgs.log_freq = saved_args["save_interval"], saved_args["log_freq"]
        logger.configure(None)
        Cfg.__dict__.clear()
        Cfg.__dict__.update(saved.__dict__)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), ckpt, "--robot", "go1", "--envs",
                          str(N), "--steps", "8", "--preset", "static_medium"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    row = json.loads(lines[0])
    assert row["preset"] == "static_medium" and row["robot"] == "go1" and row["envs"] == N and row["steps"] == 8 * N
    for k in ("lin_vel_x/mean", "lin_vel_rmsd_rms", "power_consumption/mean", "base_height/mean"):
        assert math.isfinite(row[k]), k
    assert "episodes" in row and "falls" in row and "cost_of_transport" in row
