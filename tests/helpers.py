"""Shared test helpers: configs, fixture loading, oracle state set-up."""
import contextlib
import functools
import json
import os

import numpy as np

from lrl import config as lcfg
from lrl import params as lparams
from lrl.robot import load_robot

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROBOT_FILES = {"mc": "mini_cheetah.urdf", "go1": "go1.urdf"}


def make(robot="mc", **over):
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    for k, v in over.items():
        node = cfg
        *ps, leaf = k.split(".")
        for p in ps:
            node = getattr(node, p)
        setattr(node, leaf, v)
    rob = load_robot(ROBOT_FILES[robot])
    if robot == "mc":
        cfg.terrain.x_offset = 0
    P = lparams.build_params(cfg, rob)
    M = lparams.build_model(rob)
    return cfg, rob, M, P


def make_rough(robot="go1", border_size=2.0, **over):
    """Rough-terrain variant of ``make``: trimesh ground, height scan (17 x 11 points -> 42 + 187 obs), terrain
    curriculum; the params carry terrain_mesh = 1 (contacts against lrl_sim_set_terrain's / the oracle's mesh)."""
    over = dict({"terrain.mesh_type": "trimesh", "terrain.measure_heights": True, "terrain.curriculum": True,
                 "terrain.border_size": border_size, "terrain.teleport_robots": False,
                 "env.num_observations": 42 + 187}, **over)
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    for k, v in over.items():
        node = cfg
        *ps, leaf = k.split(".")
        for p in ps:
            node = getattr(node, p)
        setattr(node, leaf, v)
    cfg.terrain.x_offset = 0
    rob = load_robot(ROBOT_FILES[robot])
    P = lparams.build_params(cfg, rob, terrain_mesh=1)
    M = lparams.build_model(rob)
    return cfg, rob, M, P


@functools.lru_cache(None)
def robot_table(name, **over):
    """(reference table in float64 of the float32 values the device gets, lrl_model, params) of "mc", "go1" or
    "go1_random_joints" (Go1 with a real fixed rotation and a general axis at every joint): the FK keys of
    aux_ref.fk and the mass tables of dyn_ref.robot.  ``over``: cfg overrides as in ``make``."""
    from lrl import _abi
    F32 = np.float32
    _, rob, M, P = make("mc" if name == "mc" else "go1", **over)
    keys = ("joint_xyz", "joint_quat", "joint_axis", "foot_xyz", "base_mass", "base_inertia", "link_mass", "link_com",
            "link_inertia")
    model = {k: np.asarray(rob[k], F32) for k in keys}
    if name == "go1_random_joints":
        rng = np.random.default_rng(11)
        jq, ja = rng.normal(size=(4, 3, 4)), rng.normal(size=(4, 3, 3))
        model["joint_quat"] = (jq / np.linalg.norm(jq, axis=-1, keepdims=True)).astype(F32)
        model["joint_axis"] = (ja / np.linalg.norm(ja, axis=-1, keepdims=True)).astype(F32)
        M2 = type(M).from_buffer_copy(M)
        M2._base = M  # (keeps the hull table the copied pointer names alive)
        _abi.fill(M2, joint_quat=model["joint_quat"].tolist(), joint_axis=model["joint_axis"].tolist())
        M = M2
    model = {k: v.astype(np.float64) for k, v in model.items()}
    model["body_leg"], model["body_link"] = list(rob["body_leg"]), list(rob["body_link"])
    return model, M, P


ALL_TERMS = {"rewards.scales.energy": -1e-3, "rewards.scales.energy_expenditure": -2e-3, "rewards.scales.dof_vel": -1e-4,
             "rewards.scales.survival": 0.3, "rewards.scales.dof_vel_limits": -0.5, "rewards.scales.torque_limits": -0.02,
             "rewards.scales.stumble": -0.4, "rewards.scales.stand_still": -0.2,
             "rewards.scales.feet_contact_forces": -0.01, "rewards.scales.orientation": -5.0,
             "rewards.scales.base_height": -30.0, "rewards.scales.termination": -2.0,
             "rewards.soft_dof_vel_limit": 0.05, "rewards.soft_torque_limit": 0.4, "rewards.max_contact_force": 20.0,
             "rewards.only_positive_rewards": False}
# (robot, fixture, cfg overrides): the presets' 12 terms for both robots, and Mini Cheetah with every _reward_* term
# of legged_robot.py:1506-1646 plus termination at a non-zero scale (make_golden.py ALL_TERMS, in that key order)
POST_PHYSICS = {"mc": ("mc", "post_physics_mc.npz", {}), "go1": ("go1", "post_physics_go1.npz", {}),
                "all_terms": ("mc", "post_physics_all_terms.npz", ALL_TERMS),
                # control_type 'V' + _push_robots every 5 steps (Go1), control_type 'T' (Mini Cheetah):
                # make_golden.py _control_tweak
                "ctl_v_push": ("go1", "post_physics_ctl_v_push.npz",
                               {"control.control_type": "V", "control.stiffness": {"joint": 2.0},
                                "control.damping": {"joint": 0.002}, "domain_rand.push_robots": True,
                                "domain_rand.push_interval_s": 0.1, "domain_rand.max_push_vel_xy": 0.5}),
                "ctl_t": ("mc", "post_physics_ctl_t.npz", {"control.control_type": "T"})}


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def init_params(module):
    """Same deterministic init as tests/golden/make_golden.py::init_params (std = 1)."""
    import zlib

    import torch
    with torch.no_grad():
        for name, p in module.named_parameters():
            r = np.random.default_rng(zlib.crc32(name.encode()))
            fan_in = p.shape[-1] if p.dim() > 1 else 1
            scale = 1.0 / np.sqrt(fan_in) if p.dim() > 1 else 0.05
            if name == "std":
                p.copy_(torch.ones_like(p))
            else:
                p.copy_(torch.tensor(r.uniform(-1, 1, tuple(p.shape)) * scale, dtype=torch.float))


def autograd_minibatch(ac, args, b, dtype, priv=None, hist=None):
    """The reference's loss (ppo.py:104-146) on one minibatch under torch autograd in ``dtype``, for either net.

    ``args`` carries clip_param, value_loss_coef, entropy_coef and use_clipped_value_loss (a PPO_Args class or any
    object with these names); ``b`` = (obs, actions, target values, returns, old log-probs, advantages, old mu, old
    sigma), the minibatch's rows.  ``priv``: the privileged rows of the teacher net (None for the plain net);
    ``hist``: the history rows — the adaptation module's regression (ppo.py:157-166) is then run as well, its
    gradients land in the same dict.  Returns a namespace: kl, value_loss, surrogate, adaptation_loss (floats),
    grads {name: grad}, and the per-row ratio and value (detached) for checks of the inputs."""
    import copy
    import types

    import torch
    import torch.nn.functional as F
    m = copy.deepcopy(ac).to(dtype)
    obs, act, tv, ret, oldlp, adv, omu, osig = (x.to(dtype) for x in b)
    priv = None if priv is None else priv.to(dtype)
    m.zero_grad(set_to_none=True)
    m.act(obs, priv)
    logp = m.get_actions_log_prob(act)
    value = m.evaluate(obs, priv)
    mu, sigma, ent = m.action_mean, m.action_std, m.entropy
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / osig + 1.e-5) + (torch.square(osig) + torch.square(omu - mu)) /
                       (2.0 * torch.square(sigma)) - 0.5, axis=-1).mean().item()
    ratio = torch.exp(logp - torch.squeeze(oldlp))
    surr = torch.max(-torch.squeeze(adv) * ratio,
                     -torch.squeeze(adv) * torch.clamp(ratio, 1 - args.clip_param, 1 + args.clip_param)).mean()
    if args.use_clipped_value_loss:
        vc = tv + (value - tv).clamp(-args.clip_param, args.clip_param)
        vl = torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
    else:
        vl = (ret - value).pow(2).mean()
    loss = surr + args.value_loss_coef * vl - args.entropy_coef * ent.mean()
    loss.backward()
    al = None
    if hist is not None:
        pred = m.adaptation_module(hist.to(dtype))
        with torch.no_grad():
            target = m.env_factor_encoder(priv)
        al = F.mse_loss(pred, target)
        al.backward()
        al = al.item()
    return types.SimpleNamespace(kl=kl, value_loss=vl.item(), surrogate=surr.item(), adaptation_loss=al,
                                 grads={k: p.grad for k, p in m.named_parameters()}, ratio=ratio.detach(),
                                 value=value.detach())


# fp32 kernel vs the fp64 oracle after the 4 sub-steps of a step, per field (atol, rtol): |got - ref| <= atol + rtol |ref|
# for every element.  Set from the measured error distribution (round 4, profiles/r4b_parity_stats.jsonl, 128 compared
# steps / 89,344 env-steps of every physics test: scripts/parity_stats_summary.py): each bar sits 2-25x above the
# largest kernel-vs-oracle error over the compared envs and about 10x above its 99.9th percentile; 4-25x tighter than
# rounds 1-3 (base position / quaternion 2e-4, joint angles 2e-3 rad, velocities 5e-2 + 1 %, contact forces 2 N + 2 %).
TOL = {"pos": (5e-5, 0.0), "quat": (1e-5, 0.0), "dof_pos": (2e-4, 0.0), "dof_vel": (2e-2, 4e-3),
       "lin_vel": (2e-3, 4e-4), "ang_vel": (5e-3, 1e-3), "contact": (0.5, 5e-3)}
# Every env must meet all of them, except envs the oracle reports as sitting on a discontinuity of the contact model
# (oracle.env_step margins: a sphere within SEP_EPS of contact_offset, a nearest-triangle or normal-rule switch within
# SEP_EPS, a restitution switch within VEL_EPS) — there fp32 and fp64 may legitimately take different branches — or
# whose fp64 result itself leaves the bars under fp32-size input noise (oracle_sensitivity).
SEP_EPS, VEL_EPS = 1e-4, 1e-3
# the margin of comparisons that start from identical state (one step, or re-synchronised steps): positions of the two
# runs differ by ~1e-7 m after the step's four sub-steps, so a branch within 1e-5 m is the most fp32 can flip
SEP_EPS_1 = 1e-5
# at most this fraction of the envs of one compared step may sit on such a discontinuity
MAX_EXCLUDED = 0.06


def within_tolerance(got, st, tol=None):
    """Per-env mask: every physics output of ``got`` within the per-field bars ``tol`` (default TOL) of ``st``."""
    tol = TOL if tol is None else tol
    n = st["root"].shape[0]

    def ok(f, a, b):
        atol, rtol = tol[f]
        err = np.abs(a - b) - rtol * np.abs(b)
        return np.all(err.reshape(n, -1) <= atol, axis=1)
    return (ok("pos", got["root"][:, :3], st["root"][:, :3]) & ok("quat", got["root"][:, 3:7], st["root"][:, 3:7])
            & ok("dof_pos", got["dof_pos"], st["dof_pos"]) & ok("dof_vel", got["dof_vel"], st["dof_vel"])
            & ok("lin_vel", got["root"][:, 7:10], st["root"][:, 7:10])
            & ok("ang_vel", got["root"][:, 10:13], st["root"][:, 10:13])
            & ok("contact", got["contact"], st["contact"]))


def physics_mismatch(got, st, margins, sensitive=None, sep_eps=SEP_EPS):
    """(bad, excluded) env masks: ``bad`` = outside tolerance and not excluded.  Excluded: the oracle's
    discontinuity margins below ``sep_eps`` / VEL_EPS, or (``sensitive``) envs whose fp64 oracle result itself leaves
    the tolerance when its input state is perturbed at float32 rounding level (see ``oracle_sensitivity``)."""
    excluded = (margins[:, 0] < sep_eps) | (margins[:, 1] < VEL_EPS)
    if sensitive is not None:
        excluded = excluded | sensitive
    return ~within_tolerance(got, st) & ~excluded, excluded


def perturb_state(st, rng, rel=2e-7):
    """A copy of an oracle state with root / joint state moved by ~float32 rounding (relative ``rel``, at least
    ``rel`` absolute): the size of the difference an fp32 restatement carries into the same step."""
    out = {k: v.copy() for k, v in st.items()}
    for k in ("root", "dof_pos", "dof_vel"):
        a = out[k]
        a += (rng.choice([-1.0, 1.0], a.shape) * rel * np.maximum(np.abs(a), 1.0)).astype(np.float32)
    return out


def oracle_sensitivity(ref, alt):
    """Envs whose oracle outputs from a perturbed start (``alt``) leave the tolerance of the unperturbed ones."""
    return ~within_tolerance(alt, ref)


# per-field views of a physics state for the error statistics
_FIELDS = {"pos": ("root", slice(0, 3)), "quat": ("root", slice(3, 7)), "dof_pos": ("dof_pos", slice(None)),
           "dof_vel": ("dof_vel", slice(None)), "lin_vel": ("root", slice(7, 10)), "ang_vel": ("root", slice(10, 13)),
           "contact": ("contact", slice(None))}


def error_stats(got, st, keep):
    """Per field: max / p99 / p50 over the kept envs of each env's largest element error |got - st| (abs) and of
    |got - st| / (1 + |st|) (scaled)."""
    out = {"envs": int(keep.sum())}
    n = st["root"].shape[0]
    for f, (k, sl) in _FIELDS.items():
        a = np.asarray(got[k], np.float64)[..., sl] if k != "contact" else np.asarray(got[k], np.float64)
        b = np.asarray(st[k], np.float64)[..., sl] if k != "contact" else np.asarray(st[k], np.float64)
        d = np.abs(a - b).reshape(n, -1)
        r = (np.abs(a - b) / (1.0 + np.abs(b))).reshape(n, -1)
        ea, er = d.max(1)[keep], r.max(1)[keep]
        if len(ea) == 0:
            continue
        out[f] = {"abs_max": float(ea.max()), "abs_p99": float(np.percentile(ea, 99)),
                  "abs_p50": float(np.percentile(ea, 50)), "scaled_max": float(er.max()),
                  "scaled_p99": float(np.percentile(er, 99))}
    return out


def record_errors(tag, got, st, excluded, alt=None):
    """Error distribution of one compared step over the non-excluded envs — kernel vs oracle, and (``alt``: the oracle
    from an fp32-rounding-size perturbed start) the fp64 oracle's own spread — appended as one JSON line to
    $LRL_PARITY_STATS when set (profiles/r4*_parity_stats.jsonl), and returned."""
    keep = ~excluded
    rec = {"tag": tag, "n": int(len(keep)), "excluded": int(excluded.sum()), "kernel_vs_oracle": error_stats(got, st, keep)}
    if alt is not None:
        rec["oracle_spread"] = error_stats(alt, st, keep)
    path = os.environ.get("LRL_PARITY_STATS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        # per-env element errors (kernel vs oracle, oracle spread) for offline analysis of tolerance choices
        arrs = {"excluded": excluded}
        for f_, (k, sl) in _FIELDS.items():
            ref = np.asarray(st[k], np.float64)
            sel = (lambda a: a[..., sl]) if k != "contact" else (lambda a: a)
            n = ref.shape[0]
            arrs["ko_" + f_] = np.abs(sel(np.asarray(got[k], np.float64)) - sel(ref)).reshape(n, -1).astype(np.float32)
            arrs["ref_" + f_] = np.abs(sel(ref)).reshape(n, -1).astype(np.float32)
            if alt is not None:
                arrs["os_" + f_] = np.abs(sel(np.asarray(alt[k], np.float64)) - sel(ref)).reshape(n, -1).astype(np.float32)
        i = sum(1 for _ in open(path)) - 1
        np.savez_compressed(path.replace(".jsonl", f"_{i:03d}.npz"), tag=np.array(tag), **arrs)
    return rec


# ---- sims made through the C ABI (lrl_sim_create) and device buffers for the kernel tests; torch is imported on use,
# so that the CPU tests that share this module do not need it ----
DEV = "cuda:0"


def vp(t):
    import ctypes as C
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32 if dtype is None else dtype, device=DEV)


def npy(t):
    return t.detach().cpu().numpy()


def stream():
    from lrl import _abi
    return _abi.stream_of(DEV)


def sync():
    import torch
    torch.cuda.synchronize()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what=""):
    """Bit-for-bit equality (NaN payloads and signed zeros included)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


class Sim:
    """An lrl_sim and torch views of its tensors."""

    def __init__(self, M, P, n, offset=0, seed=1):
        import ctypes as C

        import torch
        from lrl import _abi
        self.L = _abi.lib()
        self.h = C.c_void_p()
        self.n, self.M, self.P = n, M, P
        torch.cuda.set_device(0)
        _abi.check(self.L.lrl_sim_create(C.byref(M), C.byref(P), C.c_int32(n), C.c_int64(offset), C.c_uint64(seed),
                                         C.c_int32(0), C.byref(self.h)))
        self._views = {}

    def t(self, tid):
        import ctypes as C
        from lrl import _abi, _dlpack
        if tid not in self._views:
            d = _abi.LrlTensor()
            _abi.check(self.L.lrl_sim_tensor(self.h, C.c_int32(tid), C.byref(d)))
            self._views[tid] = _dlpack.wrap(d, 0)
        return self._views[tid]

    def close(self):
        sync()
        self.L.lrl_sim_destroy(self.h)


@contextlib.contextmanager
def sim_of(M, P, n, offset=0, seed=1):
    s = Sim(M, P, n, offset, seed)
    try:
        yield s
    finally:
        s.close()


@functools.lru_cache(None)
def _mc():
    return make("mc")


def mc_sim(n, offset=0, seed=1):
    _, _, M, P = _mc()
    return sim_of(M, P, n, offset, seed)
