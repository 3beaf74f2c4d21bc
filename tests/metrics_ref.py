"""A float64 numpy restatement of the evaluation metrics (include/lrl.h LRL_METRIC_*; the reference's METRICS_FNS):
the independent checker of tests/test_eval_metrics*.py.  Inputs are the env's public tensors as numpy arrays; every
value is formed in float64 from them."""
import numpy as np

NAMES = ("lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques",
         "power_consumption", "CoT", "froude_number", "termination")
ROWS = NAMES + ("speed_xy",)  # the tables' rows: the named metrics, then the internal row
G, LEG = 9.8, 0.30


def metrics(base_lin_vel, base_ang_vel, commands, torques, dof_vel, root_states, payloads, reset_buf,
            default_body_mass, measured_heights=0):
    """name -> float64 [n] for every row of ROWS, plus ``power_abs`` = sum_k |tau_k qd_k| and ``mass`` (the bars' scales).
    ``measured_heights``: [n, points], or the scalar 0 of an env without a height scan."""
    d = lambda a: np.asarray(a, np.float64)
    v, w, c, tq, qd, root = d(base_lin_vel), d(base_ang_vel), d(commands), d(torques), d(dof_vel), d(root_states)
    out = {}
    out["lin_vel_rmsd"] = np.sqrt((v[:, 0] - c[:, 0]) ** 2)
    out["ang_vel_rmsd"] = np.sqrt((w[:, 2] - c[:, 2]) ** 2)
    out["lin_vel_x"] = v[:, 0].copy()
    out["ang_vel_yaw"] = w[:, 2].copy()
    h = d(measured_heights)
    out["base_height"] = (root[:, 2:3] - (h if h.ndim == 2 else h.reshape(1, 1))).mean(axis=1)
    out["max_torques"] = np.abs(tq).max(axis=1)
    out["power_consumption"] = (tq * qd).sum(axis=1)
    out["power_abs"] = np.abs(tq * qd).sum(axis=1)
    out["mass"] = float(default_body_mass) + d(payloads)
    out["speed_xy"] = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["CoT"] = out["power_consumption"] / (out["mass"] * G * out["speed_xy"])
    out["froude_number"] = v[:, 0] ** 2 / (G * LEG)
    out["termination"] = d(np.asarray(reset_buf) != 0)
    return out


def bars(ref):
    """name -> the largest |got - ref| a float32 evaluation may show, per env.  Single-row metrics: the project's
    observation bar, 1e-6 relative + 1e-6 absolute; power_consumption: 1e-5 sum |tau qd| (the reward bar: a 12-term
    float32 sum); base_height: 1e-5; CoT: the power bar over m g v, plus 1e-6 |CoT| for the division."""
    one = lambda k: 1e-6 * np.abs(ref[k]) + 1e-6
    out = {k: one(k) for k in ("lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "max_torques",
                                 "froude_number", "termination", "speed_xy")}
    out["power_consumption"] = 1e-5 * ref["power_abs"]
    out["base_height"] = np.full_like(ref["base_height"], 1e-5)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["CoT"] = 1e-5 * ref["power_abs"] / (ref["mass"] * G * ref["speed_xy"]) + 1e-6 * np.abs(ref["CoT"])
    return out


def check(got, ref, rows=ROWS, what=""):
    """Assert every row of ``got`` (name -> [n]) within ``bars(ref)`` of ``ref``; a non-finite reference value (CoT at
    zero speed) must be non-finite in ``got`` too.  Returns name -> the largest error over its bar (for printing)."""
    b, worst = bars(ref), {}
    for k in rows:
        g, r = np.asarray(got[k], np.float64), ref[k]
        fin = np.isfinite(r)
        assert not np.isfinite(g[~fin]).any(), (what, k, "finite where the reference is not", g[~fin])
        err = np.abs(g[fin] - r[fin])
        worst[k] = float((err / np.maximum(b[k][fin], 1e-300)).max()) if fin.any() else 0.0
        bad = err > b[k][fin]
        assert not bad.any(), f"{what} {k}: {int(bad.sum())} envs outside the bar, worst {worst[k]:.3g} x bar"
    return worst


class Totals:
    """The per-env totals since a clear, from the per-step float32 rows: float64 sums and sums of squares in step
    order, the running float32 maximum (nan skipped), and the counters."""

    def __init__(self, n):
        self.sum = {k: np.zeros(n) for k in ROWS}
        self.sumsq = {k: np.zeros(n) for k in ROWS}
        self.abs = {k: np.zeros(n) for k in ROWS}  # sum |x| and sum x^2: the scales of the sums' bars
        self.max = {k: np.full(n, -np.inf, np.float32) for k in ROWS}
        self.steps = np.zeros(n, np.int32)
        self.episodes = np.zeros(n, np.int32)
        self.falls = np.zeros(n, np.int32)

    def add(self, step_rows, reset, time_out):
        """``step_rows``: name -> float32 [n] of one step; reset / time_out: that step's flags."""
        for k in ROWS:
            x32 = np.asarray(step_rows[k], np.float32)
            self.max[k] = np.fmax(self.max[k], x32)
            if k == "CoT":  # never accumulated
                continue
            x = x32.astype(np.float64)
            self.sum[k] = self.sum[k] + x
            self.sumsq[k] = self.sumsq[k] + x * x
            self.abs[k] = self.abs[k] + np.abs(x)
        r, t = np.asarray(reset) != 0, np.asarray(time_out) != 0
        self.steps += 1
        self.episodes += r
        self.falls += r & ~t
