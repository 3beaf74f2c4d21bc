"""ORACLE (test infrastructure only): ctypes front-end to oracle/build/liblrl_oracle.so plus numpy
restatements of the PPO bookkeeping.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the
product path (rapid-locomotion-rl_amd/) never does.

* ``env_step``         — lrl_oracle.c:lrlo_env_step (LeggedRobot.step, legged_robot.py:106-137).
* ``physics_substep``  — lrl_oracle.c:lrlo_physics_substep (own dense dynamics; PhysX parity unpinned).
* ``gae``              — RolloutStorage.compute_returns (rollout_storage.py:76-90) in numpy.
* ``reset_idx_device`` — the device part of LeggedRobot.reset_idx (legged_robot.py:227-290) in numpy float32.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "build", "liblrl_oracle.so")

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])


def _load(path):
    if not os.path.exists(path):
        build()
    L = C.CDLL(path)
    L.lrlo_env_step.restype = C.c_int
    L.lrlo_physics_substep.restype = C.c_int
    L.lrlo_energy.restype = C.c_double
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = _load(SO)
    return _lib


_cpu_lib = None


def cpu_lib():
    """The same source built in float with OpenMP over envs (oracle/Makefile liblrl_cpu.so): bench.py's CPU
    baseline; thread count from OMP_NUM_THREADS."""
    global _cpu_lib
    if _cpu_lib is None:
        _cpu_lib = _load(os.path.join(HERE, "build", "liblrl_cpu.so"))
    return _cpu_lib


ENV_FIELDS = ["root", "dof_pos", "dof_vel", "contact", "torques", "actions", "last_actions", "last_dof_vel",
              "last_root_vel", "commands", "obs", "priv", "hist", "rew", "reset", "last_contacts", "episode_length",
              "episode_sums", "command_sums", "feet_air_time", "friction", "restitution", "payload", "com",
              "motor_strength", "kp", "kd", "base_lin_vel", "base_ang_vel", "projected_gravity",
              "joint_pos_target", "heights"]


class _Env(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ENV_FIELDS]


def _dtype(f):
    return {"reset": np.uint8, "last_contacts": np.uint8, "episode_length": np.int32}.get(f, np.float32)


def make_state(n, num_bodies, num_obs, num_hist, n_es, n_cs, num_height_points=0):
    """Zero-initialised logical-layout host state."""
    shp = dict(root=(n, 13), dof_pos=(n, 12), dof_vel=(n, 12), contact=(n, num_bodies, 3), torques=(n, 12),
               actions=(n, 12), last_actions=(n, 12), last_dof_vel=(n, 12), last_root_vel=(n, 6),
               commands=(n, 4), obs=(n, num_obs), priv=(n, 18), hist=(n, num_hist * num_obs), rew=(n,),
               reset=(n,), last_contacts=(n, 4), episode_length=(n,), episode_sums=(n_es, n),
               command_sums=(n_cs, n), feet_air_time=(n, 4), friction=(n,), restitution=(n,), payload=(n,),
               com=(n, 3), motor_strength=(n, 12), kp=(n, 12), kd=(n, 12), base_lin_vel=(n, 3),
               base_ang_vel=(n, 3), projected_gravity=(n, 3), joint_pos_target=(n, 12),
               heights=(n, max(num_height_points, 1)))
    st = {k: np.zeros(v, _dtype(k)) for k, v in shp.items()}
    st["root"][:, 6] = 1.0
    st["motor_strength"][:] = 1
    st["kp"][:] = 1
    st["kd"][:] = 1
    return st


def env_step(model, params, state, actions, flags, seed=0, env_offset=0, common_step_counter=1, noise_u=None,
             dr_u=None, margins=None, library=None, push_u=None):
    """In-place LeggedRobot.step on a logical-layout state dict (see make_state).  ``margins``: optional float64
    [n, 2] array that receives each env's discontinuity margins of this step (lrl_oracle.c g_margin_*): the
    smallest |separation - contact_offset| over its spheres and sub-steps, and the smallest |u_n +
    bounce_threshold_velocity| of a contact with restitution."""
    if margins is not None:
        assert margins.dtype == np.float64 and margins.flags["C_CONTIGUOUS"] and margins.shape == (state["root"].shape[0], 2)
    L = library or lib()
    L.lrlo_set_margin_out(margins.ctypes.data_as(C.c_void_p) if margins is not None else None)
    for k in ENV_FIELDS:
        a = state[k]
        assert a.flags["C_CONTIGUOUS"] and a.dtype == _dtype(k), k
    e = _Env(**{k: state[k].ctypes.data for k in ENV_FIELDS})
    n = state["root"].shape[0]
    act = np.ascontiguousarray(actions, np.float32)
    nu = np.ascontiguousarray(noise_u, np.float32) if noise_u is not None else None
    du = np.ascontiguousarray(dr_u, np.float32) if dr_u is not None else None
    pu = np.ascontiguousarray(push_u, np.float32) if push_u is not None else None
    L.lrlo_set_push_uniforms(pu.ctypes.data_as(C.c_void_p) if pu is not None else None)
    rc = L.lrlo_env_step(C.byref(model), C.byref(params), C.c_int32(n), C.c_int64(env_offset),
                             C.c_uint64(seed), C.c_int64(common_step_counter), C.byref(e),
                             act.ctypes.data_as(C.c_void_p), C.c_uint32(flags),
                             nu.ctypes.data_as(C.c_void_p) if nu is not None else None,
                             du.ctypes.data_as(C.c_void_p) if du is not None else None)
    if rc != 0:
        raise RuntimeError("oracle env_step failed (non-SPD mass matrix)")
    L.lrlo_set_push_uniforms(None)
    return state


_terrain_keep = None


def set_terrain(vertices_world, heights_m, library=None):
    """lrl_oracle.c:lrlo_set_terrain — the terrain mesh the oracle's contacts and height scan use (params
    terrain_mesh = 1): vertices [rows, cols, 3] in the world frame, height samples [rows, cols] in metres.  Each
    build keeps its own mesh pointer (``library``: cpu_lib() for the float build), both read the same arrays."""
    global _terrain_keep
    v = np.ascontiguousarray(vertices_world, np.float32)
    h = np.ascontiguousarray(heights_m, np.float32)
    rows, cols = h.shape
    assert v.shape == (rows, cols, 3)
    _terrain_keep = (v, h)
    (library or lib()).lrlo_set_terrain(v.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), C.c_int(rows),
                                        C.c_int(cols))


def terrain_query(params, p, r):
    """lrl_oracle.c:terrain_query — (separation, world normal) of a sphere against the terrain mesh."""
    L = lib()
    L.lrlo_terrain_query.restype = C.c_double
    pp = np.ascontiguousarray(p, np.float64).reshape(3)
    n = np.zeros(3, np.float64)
    sep = L.lrlo_terrain_query(C.byref(params), pp.ctypes.data_as(C.c_void_p), C.c_double(r),
                               n.ctypes.data_as(C.c_void_p))
    return sep, n


def height_sample(params, root, k):
    lib().lrlo_height_sample.restype = C.c_float
    r = np.ascontiguousarray(root, np.float32).reshape(13)
    return lib().lrlo_height_sample(C.byref(params), r.ctypes.data_as(C.c_void_p), C.c_int(k))


def physics_substep(model, params, root, q, qd, tau, friction, restitution, payload, com, library=None):
    """lrl_oracle.c:lrlo_physics_substep — one cold-started sub-step of one env: (root, q, qd, contact forces [B, 3],
    number of active ground contacts).  ``library``: cpu_lib() for the float build."""
    f = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
    root, q, qd, tau, com = f(root, 13), f(q, 12), f(qd, 12), f(tau, 12), f(com, 3)
    ro, qo, qdo = np.zeros(13, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    co = np.zeros((model.num_bodies, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = (library or lib()).lrlo_physics_substep(C.byref(model), C.byref(params), p(root), p(q), p(qd), p(tau),
                                                C.c_float(friction), C.c_float(restitution), C.c_float(payload), p(com),
                                                p(ro), p(qo), p(qdo), p(co))
    return ro, qo, qdo, co, n


def self_pairs(model, q=None):
    """lrl_oracle.c:lrlo_self_pairs: the self-collision candidate pairs [n, 2] (b = -1: the base box) in the canonical
    order and, for joint angles q [12] (default 0), their separations [n]."""
    L = lib()
    pairs = np.zeros((256, 2), np.int32)
    sep = np.zeros(256, np.float64)
    qa = None if q is None else np.ascontiguousarray(q, np.float32)
    n = L.lrlo_self_pairs(C.byref(model), None if qa is None else qa.ctypes.data_as(C.c_void_p),
                          pairs.ctypes.data_as(C.c_void_p), sep.ctypes.data_as(C.c_void_p))
    return pairs[:n].copy(), sep[:n].copy()


def energy(model, params, root, q, qd, payload=0.0, com=(0, 0, 0)):
    f = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    root, q, qd, com = f(root, 13), f(q, 12), f(qd, 12), f(com, 3)
    return lib().lrlo_energy(C.byref(model), C.byref(params), p(root), p(q), p(qd), C.c_float(payload), p(com))


def gae(rewards, dones, values, last_values, gamma, lam):
    """rollout_storage.py:76-90 in numpy float32 (same recurrence and normalisation)."""
    T = rewards.shape[0]
    rewards, values = rewards.astype(np.float32), values.astype(np.float32)
    returns = np.zeros_like(values)
    adv = np.zeros_like(values[0])
    g, gl = np.float32(gamma), np.float32(gamma * lam)
    for t in reversed(range(T)):
        nv = last_values.astype(np.float32) if t == T - 1 else values[t + 1]
        nt = np.float32(1.0) - dones[t].astype(np.float32)
        delta = rewards[t] + nt * g * nv - values[t]
        adv = delta + nt * gl * adv
        returns[t] = adv + values[t]
    a = returns - values
    return returns, (a - a.mean(dtype=np.float64)) / (a.std(ddof=1, dtype=np.float64) + 1e-8)


def reset_idx_device(params, state, ids, u, root_mode, xy_lo=0.0, xy_span=0.0, x_off=0.0, y_off=0.0):
    """reset_idx's per-env state changes (legged_robot.py:244-259) on a logical-layout state dict, in place:
    _randomize_dof_props (:544-560: rand * (max - min) + min, two float32 roundings), _reset_dofs (:690-712),
    _reset_root_states (:714-755; root_mode as lrl.h: 0 fork custom origins (Q4), 1 base_init_state + origin,
    2 upstream custom origins with the xy draw and init offsets), then last_actions / last_dof_vel / feet_air_time /
    episode_length zeroed and reset_buf set.  u [len(ids), 5]: (motor strength, Kp, Kd, x, y) uniforms."""
    f32 = np.float32
    ids = np.asarray(ids)
    u = np.asarray(u, f32)
    span = [f32(s) for s in params.dr_span]
    for flag, key, lo, j in ((params.randomize_motor_strength, "motor_strength", params.motor_strength_range[0], 0),
                             (params.randomize_kp, "kp", params.kp_range[0], 1),
                             (params.randomize_kd, "kd", params.kd_range[0], 2)):
        if flag:
            state[key][ids] = ((u[:, j] * span[j]).astype(f32) + f32(lo)).astype(f32)[:, None]
    state["dof_pos"][ids] = np.array(params.default_dof_pos[:], f32)
    state["dof_vel"][ids] = 0.0
    if root_mode != 0:
        r = np.tile(np.array(params.base_init_state[:], f32), (len(ids), 1))
        r[:, :3] = r[:, :3] + state["env_origins"][ids]
        if root_mode == 2:
            xy = (f32(xy_span) * u[:, 3:5]).astype(f32) + f32(xy_lo)
            r[:, :2] = r[:, :2] + xy
            r[:, 0] = r[:, 0] + f32(x_off)
            r[:, 1] = r[:, 1] + f32(y_off)
        state["root"][ids] = r
    for k in ("last_actions", "last_dof_vel", "feet_air_time"):
        state[k][ids] = 0.0
    state["episode_length"][ids] = 0
    state["reset"][ids] = 1
    return state


def set_solver_tgs(on):
    """lrl_oracle.c:lrlo_set_solver_tgs — the PGS-vs-TGS study's solver switch (scripts/tgs_vs_pgs.py); 0 (the model
    the kernel runs) everywhere else."""
    lib().lrlo_set_solver_tgs(C.c_int(1 if on else 0))
