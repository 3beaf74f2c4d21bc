"""Evaluation metrics accumulated on the device (include/lrl.h lrl_sim_metrics_*, csrc/lrl_metrics.hip).

The reference's ``mini_gym_learn/eval_metrics/metrics.py`` computes each metric with one device -> host copy per metric
and step.  Here one small kernel per env step writes the same values into a per-step table and adds them to per-env
totals (fp64 sums and sums of squares, fp32 maxima, step / episode / fall counts); ``summary`` pools a group of envs
with one reduction launch and one read.

    m = EvalMetrics(env)          # env: LeggedRobotEnv or a wrapper holding one as .env
    m.enable(); m.clear()
    ... env.step(actions) ...
    m.summary("eval")             # {"lin_vel_x/mean": ..., "cost_of_transport": ..., "episodes": ..., ...}

The cost of transport of a group is sum P / (9.8 sum_e m_e sum_t |v_xy|): total energy over total weight x distance,
from the sums; the per-step ``CoT`` row (the reference's P / (m g |v_xy|), inf / nan at zero speed) is never added up.
"""
import ctypes as C
import math

import torch

from . import _abi, _dlpack

NAMES = _abi.METRIC_NAMES
GRAVITY = 9.8  # the reference's g of CoT / froude_number (not Cfg.sim.gravity)


class EvalMetrics:
    def __init__(self, env):
        while not hasattr(env, "_sim") and hasattr(env, "env"):  # HistoryWrapper and the like
            env = env.env
        if not hasattr(env, "_sim"):
            raise TypeError("EvalMetrics needs a native env (lrl.env.LeggedRobotEnv)")
        self.env = env
        self._L = env._L
        self._view = None
        self._out = None
        self.enabled = False

    # ---- switches
    def enable(self):
        """Launch the metrics kernel in every later step (the first call allocates the tables, totals cleared)."""
        _abi.check(self._L.lrl_sim_metrics_enable(self.env._sim, 1))
        self.enabled = True
        self._tables()
        return self

    def disable(self):
        _abi.check(self._L.lrl_sim_metrics_enable(self.env._sim, 0))
        self.enabled = False

    def clear(self):
        """Zero the totals (sums 0, maxima -inf, counts 0) on the env's stream."""
        self._tables()
        _abi.check(self._L.lrl_sim_metrics_clear(self.env._sim, self.env._stream()))

    # ---- zero-copy views
    def _tables(self):
        if self._view is None:
            v = _abi.LrlMetricsView()
            _abi.check(self._L.lrl_sim_metrics_tensors(self.env._sim, C.byref(v)))
            n, R, pitch = v.num_envs, v.rows, v.pitch

            def wrap(ptr, dtype, rows):
                d = _abi.LrlTensor()
                d.data, d.dtype, d.ndim = ptr, dtype, 2 if rows else 1
                if rows:
                    d.shape[0], d.shape[1], d.strides[0], d.strides[1] = rows, pitch, pitch, 1
                else:
                    d.shape[0], d.strides[0] = pitch, 1
                return _dlpack.wrap(d, self.env._dev_index)
            # the whole allocation (rows of `pitch` elements, the padded env count); the kernels write the first n
            self._full = dict(step=wrap(v.step, 0, R), sum=wrap(v.sum, _dlpack.F64, R), sumsq=wrap(v.sumsq, _dlpack.F64, R),
                              max=wrap(v.max, 0, R), steps=wrap(v.steps, 1, 0), episodes=wrap(v.episodes, 1, 0),
                              falls=wrap(v.falls, 1, 0))
            self._view = {k: t[..., :n] for k, t in self._full.items()}
            self.pitch, self.rows = pitch, R
        return self._view

    def tables(self, padded=False):
        """The raw tables as views: step / sum / sumsq / max [rows, num_envs] (rows in ``_abi.METRIC_NAMES`` order, then
        the internal ``speed_xy`` row), steps / episodes / falls [num_envs].  ``padded``: the whole rows instead, [rows,
        pitch] / [pitch] with pitch the padded env count; the lanes past num_envs are never written."""
        self._tables()
        return dict(self._full if padded else self._view)

    def step_values(self):
        """name -> [num_envs] float32 view of the last step's values."""
        step = self._tables()["step"]
        return {k: step[i] for i, k in enumerate(NAMES)}

    def per_env(self):
        """Per-env statistics since the last clear, device tensors: ``{name}/mean``, ``/std`` (population), ``/max``
        (max only for CoT), ``cost_of_transport``, ``steps``, ``episodes``, ``falls``."""
        t = self._tables()
        steps = t["steps"].to(torch.float64)
        out = {}
        for i, k in enumerate(NAMES):
            out[k + "/max"] = t["max"][i]
            if k == "CoT":
                continue
            mean = t["sum"][i] / steps
            out[k + "/mean"] = mean
            out[k + "/std"] = torch.sqrt(torch.clamp(t["sumsq"][i] / steps - mean * mean, min=0.0))
        mass = (torch.tensor(self.env.default_body_mass, dtype=torch.float32, device=steps.device)
                + self.env.payloads).to(torch.float64)
        out["cost_of_transport"] = t["sum"][NAMES.index("power_consumption")] / \
            (mass * GRAVITY * t["sum"][_abi.METRIC_SPEED_XY])
        out["steps"], out["episodes"], out["falls"] = t["steps"], t["episodes"], t["falls"]
        return out

    # ---- pooled over a group
    def group_range(self, group):
        e = self.env
        if group == "train":
            return 0, e.num_train_envs
        if group == "eval":
            return e.num_train_envs, e.num_envs - e.num_train_envs
        if group == "all":
            return 0, e.num_envs
        raise ValueError(f"group must be 'train', 'eval' or 'all', got {group!r}")

    def reduce(self, group="all"):
        """The raw reduction (lrl_sim_metrics_reduce) of a group as a host float64 tensor: one launch, one read."""
        self._tables()
        first, count = self.group_range(group)
        if self._out is None:
            self._out = torch.empty(_abi.METRICS_REDUCE_DOUBLES, dtype=torch.float64, device=self.env.device)
        _abi.check(self._L.lrl_sim_metrics_reduce(self.env._sim, first, count, self._out.data_ptr(),
                                                  self.env._stream()))
        return self._out.cpu()

    def summary(self, group="all"):
        """A plain dict of the group's pooled statistics over its env-steps since the last clear: per metric
        ``{name}/mean``, ``/std``, ``/max`` (``CoT``: max only), ``lin_vel_rmsd_rms`` (the true RMSD: the square root of
        the mean squared error), ``cost_of_transport``, ``episodes``, ``falls``, ``steps``."""
        r = self.reduce(group).tolist()
        R = _abi.METRIC_ROWS
        steps, episodes, falls, weight_dist = r[3 * R:3 * R + 4]
        out = {}
        for i, k in enumerate(NAMES):
            s, ss, mx = r[3 * i:3 * i + 3]
            if k != "CoT":
                mean = s / steps if steps else math.nan
                out[k + "/mean"] = mean
                out[k + "/std"] = math.sqrt(max(ss / steps - mean * mean, 0.0)) if steps else math.nan
            out[k + "/max"] = mx
        i = NAMES.index("lin_vel_rmsd")
        out["lin_vel_rmsd_rms"] = math.sqrt(r[3 * i + 1] / steps) if steps else math.nan
        power = r[3 * NAMES.index("power_consumption")]
        out["cost_of_transport"] = power / (GRAVITY * weight_dist) if weight_dist else math.nan
        out["episodes"], out["falls"], out["steps"] = int(episodes), int(falls), int(steps)
        return out
