"""The eval group's own domain-randomisation, push and teleport parameters on the device (lrl_sim_set_eval_group,
lrl_sim_randomize_envs; LeggedRobotEnv(cfg, eval_cfg)): what the reference runs under _call_train_eval with the
group's cfg (legged_robot.py:456-469).  Shapes put both groups into one wave: 6 + 7 envs on the plane build (4 envs per
wave), 18 + 9 on the terrain-mesh builds (16 per wave)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import POST_PHYSICS, Sim, golden, make, mc_sim, same
from lrl import _abi
from lrl import config as lcfg
from lrl import params as lparams

pytestmark = pytest.mark.gpu

f32 = np.float32
INJECT = _abi.STEP_INJECT_UNIFORM


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    return _abi.stream_of("cuda:0")


def _cfg(robot, n, **over):
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    cfg.env.num_envs = n
    lcfg._apply(cfg, over)
    return cfg


def _split(robot, n_tr, over_tr, n_ev, over_ev, **kw):
    from lrl.env import LeggedRobotEnv
    return LeggedRobotEnv("cuda:0", cfg=_cfg(robot, n_tr, **over_tr), eval_cfg=_cfg(robot, n_ev, **over_ev), **kw)


def _step(L, sim, stream, act, flags, noise=None, dr=None, push=None):
    if noise is not None:
        _abi.check(L.lrl_sim_inject_uniforms(sim, C.c_void_p(noise.data_ptr()), C.c_void_p(dr.data_ptr())))
    if push is not None:
        _abi.check(L.lrl_sim_inject_push_uniforms(sim, C.c_void_p(push.data_ptr())))
    _abi.check(L.lrl_sim_step(sim, C.c_void_p(act.data_ptr()), C.c_uint32(flags), stream))
    torch.cuda.synchronize()


def _group_of(P, G, rows_eval, n):
    """Per env: the block its group reads (P for the train rows, G for the eval rows)."""
    return [G if rows_eval[e] else P for e in range(n)]


def _draw(u, span, lo):
    """torch.rand * (max - min) + min in float32: two roundings."""
    return f32(f32(u) * f32(span)) + f32(lo)


def _expected_group_rows(blocks, rand_interval, eplen_in, ms_in, vel_in, dr_u, push_u):
    """The numpy restatement for one step of identity physics: per env the motor strength after the DR redraw
    (:544-560, :591-593), the root x / y velocity after _push_robots (:757-766), and which envs redrew."""
    n = len(blocks)
    L = eplen_in.astype(np.int64) + 1
    redraw = (L % rand_interval) == 0
    ms, vel = ms_in.copy(), vel_in.copy()
    pushed = np.zeros(n, bool)
    for e, B in enumerate(blocks):
        if redraw[e] and B.randomize_motor_strength:
            ms[e, :] = _draw(dr_u[e], B.dr_span[0], B.motor_strength_range[0])
        if B.push_robots and L[e] % B.push_interval == 0:
            pushed[e] = True
            for c in range(2):
                vel[e, c] = f32(f32(B.push_span) * f32(push_u[e, c])) + f32(B.push_lo)
    return ms, vel, redraw, pushed


def _check_group_rows(blocks, rows, rand_interval, before, after, dr_u, push_u, what):
    """`rows`: the env rows to check; before / after: dicts of eplen, ms, kp, kd, root numpy arrays (all envs)."""
    ms, vel, redraw, pushed = _expected_group_rows(blocks, rand_interval, before["eplen"], before["ms"],
                                                   before["root"][:, 7:9], dr_u, push_u)
    same(after["ms"][rows], ms[rows], what + " motor strengths")
    same(after["root"][rows, 7:9], vel[rows], what + " pushed root velocity")
    same(after["root"][rows, :7], before["root"][rows, :7], what + " root pose")  # (identity physics, no teleport here)
    for k, sw, rng in (("kp", "randomize_kp", "kp_range"), ("kd", "randomize_kd", "kd_range")):
        for e in np.flatnonzero(rows):
            B = blocks[e]
            if redraw[e] and getattr(B, sw):
                lo, hi = getattr(B, rng)
                v = after[k][e]
                assert np.all(v == v[0]) and f32(lo) <= v[0] <= f32(hi), (what, k, e, v[0], lo, hi)
            else:
                same(after[k][e], before[k][e], f"{what} {k} of env {e} (no redraw)")
    return redraw, pushed


class _Views:
    """Numpy snapshots of a sim's per-env state through its tensor getter."""

    def __init__(self, t):
        self.t = t

    def snap(self):
        t = self.t
        return dict(eplen=_np(t(_abi.T_EPISODE_LENGTH)), ms=_np(t(_abi.T_MOTOR_STRENGTH)), kp=_np(t(_abi.T_KP_FACTOR)),
                    kd=_np(t(_abi.T_KD_FACTOR)), root=_np(t(_abi.T_ROOT_STATE)))


# ---------------------------------------------------------------------------------------------- reference replay
# Y differs from the fixture's cfg X in every per-group DR / push field: each switch flipped, every range, the push
# interval and velocity changed
def _other_group(cfg_x):
    d = cfg_x.domain_rand
    return {"domain_rand.randomize_motor_strength": not d.randomize_motor_strength,
            "domain_rand.randomize_Kp_factor": not d.randomize_Kp_factor,
            "domain_rand.randomize_Kd_factor": not d.randomize_Kd_factor,
            "domain_rand.motor_strength_range": [0.4, 0.6], "domain_rand.Kp_factor_range": [1.5, 1.75],
            "domain_rand.Kd_factor_range": [2.0, 2.5], "domain_rand.push_robots": not d.push_robots,
            "domain_rand.push_interval_s": 0.3 if d.push_robots else 0.1, "domain_rand.max_push_vel_xy": 0.9}


# episode lengths of the Y rows: redraws (a multiple of rand_interval 301 after the increment) at steps 0 and 1, pushes
# (multiples of 6) at steps 0, 1 and 2, and both at once (3612 = 12 x 301 = 602 x 6)
Y_EPLEN = np.array([300, 299, 5, 4, 3, 3611], np.int32)


@pytest.mark.parametrize("swapped", [False, True], ids=["x_is_eval", "x_is_train"])
@pytest.mark.parametrize("case", ["mc", "ctl_v_push"])
def test_post_physics_replay_in_a_split_sim(case, swapped):
    """tests/test_env_gpu.py::test_post_physics_matches_reference on the rows of one group of a split sim whose other
    group (m = 6 envs) has different DR / push parameters: the fixture's rows must equal the reference's recorded
    arrays under that test's comparisons; the other rows follow their own group's values (numpy restatement)."""
    robot, fixture, over = POST_PHYSICS[case]
    g = golden(fixture)
    n, m = g["root_in"].shape[1], len(Y_EPLEN)
    cfg_x, _, M, PX = make(robot, **over)
    _, _, _, PY = make(robot, **dict(over, **_other_group(cfg_x)))
    for f, a, b in (("randomize_motor_strength", PX, PY), ("randomize_kp", PX, PY), ("randomize_kd", PX, PY),
                    ("push_robots", PX, PY), ("push_interval", PX, PY), ("push_span", PX, PY)):
        assert getattr(a, f) != getattr(b, f), f
    Ptr, Pev = (PX, PY) if swapped else (PY, PX)
    n_tr = n if swapped else m
    N = n + m
    G = lparams.eval_group_params(Ptr, Pev)
    assert G is not None
    Ptr.num_train_envs = n_tr
    xr = np.zeros(N, bool)
    xr[(slice(0, n) if swapped else slice(m, N))] = True
    yr = ~xr
    rows_eval = np.arange(N) >= n_tr
    blocks = _group_of(Ptr, G, rows_eval, N)
    rng = np.random.default_rng(31)

    def full(a, axis=0):
        """Golden rows into the X rows, copies of its rows 5 .. 5 + m into the Y rows (rows whose positions lie
        inside the tiles: the Mini Cheetah fixture teleports rows 0, 1, 2, 4 and 11)."""
        a = np.asarray(a)
        out = np.zeros(a.shape[:axis] + (N,) + a.shape[axis + 1:], a.dtype)
        ix = [slice(None)] * a.ndim
        ix[axis] = xr
        out[tuple(ix)] = a
        iy, src = list(ix), list(ix)
        iy[axis], src[axis] = yr, slice(5, 5 + m)
        out[tuple(iy)] = a[tuple(src)]
        return out

    s = Sim(M, Ptr, N)
    try:
        L, t = s.L, s.t
        _abi.check(L.lrl_sim_set_eval_group(s.h, C.byref(G)))
        st = _stream()
        t(_abi.T_FRICTION)[:] = _dev(full(g["init_friction"]))
        t(_abi.T_RESTITUTION)[:] = _dev(full(g["init_restitution"]))
        t(_abi.T_PAYLOAD)[:] = _dev(full(g["init_payload"]))
        t(_abi.T_COM_DISPLACEMENT)[:] = _dev(full(g["init_com"]))
        t(_abi.T_MOTOR_STRENGTH)[:] = _dev(full(g["init_motor_strengths"]))
        t(_abi.T_KP_FACTOR)[:] = 1.0
        t(_abi.T_KD_FACTOR)[:] = 1.0
        ep = full(g["init_episode_length"])
        ep[yr] = Y_EPLEN
        t(_abi.T_EPISODE_LENGTH)[:] = _dev(ep, torch.int32)
        t(_abi.T_EPISODE_SUMS)[:] = _dev(full(g["init_episode_sums"], 1))
        t(_abi.T_COMMAND_SUMS)[:] = _dev(full(g["init_command_sums"], 1))
        t(_abi.T_FEET_AIR_TIME)[:] = _dev(full(g["init_feet_air_time"]))
        t(_abi.T_LAST_CONTACTS)[:] = _dev(full(g["init_last_contacts"]), torch.uint8)
        t(_abi.T_LAST_ACTIONS)[:] = _dev(full(g["init_last_actions"]))
        t(_abi.T_LAST_DOF_VEL)[:] = _dev(full(g["init_last_dof_vel"]))
        V = _Views(t)
        seen_redraw = seen_push = 0
        for k in range(g["root_in"].shape[0]):
            t(_abi.T_ROOT_STATE)[:] = _dev(full(g["root_in"][k]))
            t(_abi.T_DOF_POS)[:] = _dev(full(g["dof_pos_in"][k]))
            t(_abi.T_DOF_VEL)[:] = _dev(full(g["dof_vel_in"][k]))
            t(_abi.T_CONTACT_FORCE)[:] = _dev(full(g["contact_in"][k]))
            t(_abi.T_COMMANDS)[:] = _dev(full(g["commands"][k]))
            dr_u = full(np.nan_to_num(g["ms_u"][k]))
            dr_u[yr] = rng.random(m, dtype=f32)
            push_u = full(np.nan_to_num(g["push_u"][k])) if "push_u" in g.files else np.zeros((N, 2), f32)
            push_u[yr] = rng.random((m, 2), dtype=f32)
            before = V.snap()
            keep = [_dev(full(g["actions"][k])), _dev(full(g["noise_u"][k])), _dev(dr_u), _dev(push_u)]
            _step(L, s.h, st, keep[0], INJECT, keep[1], keep[2], keep[3])
            after = V.snap()
            # -- the fixture's rows: the reference's recorded arrays, test_post_physics_matches_reference's comparisons
            X = lambda tid: _np(t(tid))[xr]
            np.testing.assert_array_equal(X(_abi.T_TORQUES), g["torques"][k])
            np.testing.assert_array_equal(X(_abi.T_JOINT_POS_TARGET), g["joint_pos_target"][k])
            np.testing.assert_array_equal(X(_abi.T_ROOT_STATE), g["root_out"][k])
            np.testing.assert_array_equal(X(_abi.T_MOTOR_STRENGTH), g["motor_strengths"][k])
            np.testing.assert_array_equal(X(_abi.T_RESET), g["reset"][k])
            np.testing.assert_array_equal(X(_abi.T_EPISODE_LENGTH), g["episode_length"][k])
            np.testing.assert_array_equal(X(_abi.T_LAST_CONTACTS).astype(bool), g["last_contacts"][k])
            tol = dict(rtol=2e-6, atol=2e-6)
            np.testing.assert_allclose(X(_abi.T_BASE_LIN_VEL), g["base_lin_vel"][k], **tol)
            np.testing.assert_allclose(X(_abi.T_BASE_ANG_VEL), g["base_ang_vel"][k], **tol)
            np.testing.assert_allclose(X(_abi.T_PROJECTED_GRAVITY), g["projected_gravity"][k], **tol)
            np.testing.assert_allclose(X(_abi.T_FEET_AIR_TIME), g["feet_air_time"][k], **tol)
            np.testing.assert_allclose(X(_abi.T_REWARD), g["rew"][k], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(_np(t(_abi.T_EPISODE_SUMS))[:, xr], g["episode_sums"][k], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(_np(t(_abi.T_COMMAND_SUMS))[:, xr], g["command_sums"][k], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(X(_abi.T_OBS), g["obs"][k], rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(X(_abi.T_PRIV_OBS), g["priv"][k], rtol=1e-6, atol=1e-6)
            # X randomises neither Kp nor Kd: the other group's switches do not reach its rows
            assert np.all(after["kp"][xr] == 1.0) and np.all(after["kd"][xr] == 1.0)
            # -- the other group's rows: their own switches, ranges, interval and velocity
            rd, pu = _check_group_rows(blocks, yr, Ptr.rand_interval, before, after, dr_u, push_u, f"step {k} Y")
            seen_redraw += int(rd[yr].sum())
            seen_push += int(pu[yr].sum())
        assert seen_redraw >= 3  # the Y rows did redraw, and (where Y pushes) were pushed on several steps
        assert seen_push >= (4 if PY.push_robots else 0)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- both groups' own values
ROUGH = {"terrain.mesh_type": "trimesh", "terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2],
         "terrain.terrain_noise_magnitude": 0.05, "terrain.border_size": 2.0, "terrain.num_rows": 3,
         "terrain.num_cols": 3, "terrain.terrain_length": 4.0, "terrain.terrain_width": 4.0,
         "terrain.max_init_terrain_level": 2, "terrain.teleport_robots": False}
GROUP_A = {"domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": [0.4, 0.6],
           "domain_rand.randomize_Kp_factor": True, "domain_rand.Kp_factor_range": [0.5, 0.6],
           "domain_rand.randomize_Kd_factor": True, "domain_rand.Kd_factor_range": [0.2, 0.3],
           "domain_rand.push_robots": True, "domain_rand.push_interval_s": 0.1, "domain_rand.max_push_vel_xy": 0.5}
GROUP_B = {"domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": [1.2, 1.5],
           "domain_rand.randomize_Kp_factor": True, "domain_rand.Kp_factor_range": [1.5, 1.7],
           "domain_rand.randomize_Kd_factor": True, "domain_rand.Kd_factor_range": [2.0, 2.4],
           "domain_rand.push_robots": True, "domain_rand.push_interval_s": 0.07, "domain_rand.max_push_vel_xy": 0.9}
BUILDS = {"plane": ("go1", 6, 7, {}), "mesh_pgs": ("go1", 18, 9, ROUGH),
          "mesh_tgs": ("go1", 18, 9, dict(ROUGH, **{"sim.physx.terrain_solver_type": 1}))}


def _build_of(env):
    return "plane" if not env._P.terrain_mesh else ("mesh_tgs" if env._P.solver_tgs else "mesh_pgs")


@pytest.mark.parametrize("build", list(BUILDS))
def test_each_group_redraws_and_pushes_with_its_own_values(build):
    """Motor strengths after a redraw step equal float32(u * span_g) + lo_g, the pushed root velocity equals
    push_span_g * u + push_lo_g on exactly the steps where (episode_length + 1) % push_interval_g == 0, bit for bit;
    Kp / Kd (no injection) land inside their own group's range (the groups' ranges are disjoint)."""
    robot, n_tr, n_ev, base = BUILDS[build]
    env = _split(robot, n_tr, dict(base, **GROUP_A), n_ev, dict(base, **GROUP_B))
    try:
        assert _build_of(env) == build
        P, G, N = env._P, env._G, n_tr + n_ev
        assert G is not None and (P.push_interval, G.push_interval) == (6, 4) and P.rand_interval == 301
        blocks = _group_of(P, G, np.arange(N) >= n_tr, N)
        rng = np.random.default_rng(7)
        # redraws at steps 0 / 1 / 2 (300, 299, 298), pushes of either interval at each step, both at once (3611)
        pool = np.array([300, 299, 298, 5, 4, 3, 2, 3611, 11, 601], np.int32)
        env.episode_length_buf[:] = _dev(pool[np.arange(N) % len(pool)], torch.int32)
        env.root_states[:, 7:13] = _dev(rng.normal(size=(N, 6)).astype(f32) * 0.1)
        V = _Views(env._tensor)
        act = torch.zeros(N, 12, device="cuda:0")
        noise = _dev(rng.random((N, P.num_obs), dtype=f32))
        seen = np.zeros((2, 2), int)
        for k in range(3):
            dr_u, push_u = rng.random(N, dtype=f32), rng.random((N, 2), dtype=f32)
            before = V.snap()
            keep = (_dev(dr_u), _dev(push_u))
            _step(env._L, env._sim, env._stream(), act, INJECT, noise, keep[0], keep[1])
            after = V.snap()
            rd, pu = _check_group_rows(blocks, np.ones(N, bool), P.rand_interval, before, after, dr_u, push_u,
                                       f"{build} step {k}")
            for gi, rows in enumerate((np.arange(N) < n_tr, np.arange(N) >= n_tr)):
                seen[gi] += (int(rd[rows].sum()), int(pu[rows].sum()))
        assert (seen >= 2).all(), seen  # both groups redrew and were pushed
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- reset
def test_reset_idx_redraws_each_env_with_its_group():
    tr = {"domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": [0.4, 0.6],
          "domain_rand.randomize_Kp_factor": False, "domain_rand.Kp_factor_range": [0.5, 0.6],
          "domain_rand.randomize_Kd_factor": True, "domain_rand.Kd_factor_range": [0.2, 0.3]}
    ev = {"domain_rand.randomize_motor_strength": False, "domain_rand.motor_strength_range": [1.2, 1.5],
          "domain_rand.randomize_Kp_factor": True, "domain_rand.Kp_factor_range": [1.5, 1.7],
          "domain_rand.randomize_Kd_factor": True, "domain_rand.Kd_factor_range": [2.0, 2.4]}
    n_tr, n_ev = 6, 7
    env = _split("mc", n_tr, tr, n_ev, ev)
    try:
        N, P, G = n_tr + n_ev, env._P, env._G
        rng = np.random.default_rng(3)
        prev = {k: (rng.random((N, 12), dtype=f32) + 3.0) for k in ("ms", "kp", "kd")}
        env.motor_strengths[:], env.Kp_factors[:], env.Kd_factors[:] = (_dev(prev[k]) for k in ("ms", "kp", "kd"))
        ids = np.array([1, 8, 5, 12, 6, 0, 10])  # both groups, interleaved, the boundary envs 5 and 6 among them
        u = rng.random((len(ids), 5), dtype=f32)
        env.reset_uniforms = _dev(u)
        env.reset_idx(torch.as_tensor(ids, device="cuda:0"))
        torch.cuda.synchronize()
        got = dict(ms=_np(env.motor_strengths), kp=_np(env.Kp_factors), kd=_np(env.Kd_factors))
        want = {k: v.copy() for k, v in prev.items()}
        for i, e in enumerate(ids):
            B = G if e >= n_tr else P
            for j, (k, sw, rg) in enumerate((("ms", "randomize_motor_strength", "motor_strength_range"),
                                             ("kp", "randomize_kp", "kp_range"), ("kd", "randomize_kd", "kd_range"))):
                if getattr(B, sw):  # (a switch that is off keeps the previous values)
                    want[k][e, :] = _draw(u[i, j], B.dr_span[j], getattr(B, rg)[0])
        for k in want:
            same(got[k], want[k], k)
        assert not np.array_equal(want["ms"][1], prev["ms"][1]) and np.array_equal(want["ms"][8], prev["ms"][8])
        assert np.array_equal(want["kp"][1], prev["kp"][1]) and not np.array_equal(want["kp"][8], prev["kp"][8])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- creation
def test_creation_draws_rigid_body_properties_per_group():
    from lrl.env import LeggedRobotEnv
    tr = {"domain_rand.friction_range": [0.1, 0.2], "domain_rand.restitution_range": [0.0, 0.1],
          "domain_rand.added_mass_range": [-1.0, 0.0], "domain_rand.com_displacement_range": [-0.1, -0.05]}
    ev = {"domain_rand.friction_range": [2.0, 3.0], "domain_rand.restitution_range": [0.5, 0.9],
          "domain_rand.added_mass_range": [1.0, 3.0], "domain_rand.com_displacement_range": [0.05, 0.1],
          "domain_rand.randomize_restitution": False}
    n_tr, n_ev = 6, 7
    N = n_tr + n_ev
    env = _split("mc", n_tr, tr, n_ev, ev, seed=5)
    one = LeggedRobotEnv("cuda:0", cfg=_cfg("mc", N, **tr), seed=5)
    with mc_sim(N) as raw:  # a sim nothing was drawn for: the initial values
        rest0 = _np(raw.t(_abi.T_RESTITUTION))
    try:
        assert env._G is None  # nothing per-step differs: the creation draw alone honours the eval cfg
        got = {k: _np(getattr(env, k)) for k in ("friction_coeffs", "restitutions", "payloads", "com_displacements")}
        ref = {k: _np(getattr(one, k)) for k in got}
        for k in got:  # the keys are global env ids: the train rows are those of a sim without an eval group
            same(got[k][:n_tr], ref[k][:n_tr], k)
        inside = lambda a, r: bool(np.all((a >= f32(r[0])) & (a <= f32(r[1]))))
        for rows, c in ((slice(0, n_tr), tr), (slice(n_tr, N), ev)):
            assert inside(got["friction_coeffs"][rows], c["domain_rand.friction_range"])
            assert inside(got["payloads"][rows], c["domain_rand.added_mass_range"])
            assert inside(got["com_displacements"][rows], c["domain_rand.com_displacement_range"])
        assert inside(got["restitutions"][:n_tr], tr["domain_rand.restitution_range"])
        same(got["restitutions"][n_tr:], rest0[n_tr:], "eval restitution (switch off)")
        assert len(np.unique(got["friction_coeffs"])) == N  # every env its own draw
    finally:
        env.close()
        one.close()


def test_randomize_envs_draws_what_randomize_draws():
    """An env draws the same uniforms whichever call covers it; envs outside the range keep their values."""
    arr = lambda a, b: (C.c_float * 2)(a, b)
    r = (arr(0.1, 0.9), arr(0.2, 0.4), arr(-1.0, 2.0), arr(-0.1, 0.1))
    ids = (_abi.T_FRICTION, _abi.T_RESTITUTION, _abi.T_PAYLOAD, _abi.T_COM_DISPLACEMENT)
    N = 13
    with mc_sim(N, offset=32, seed=9) as a, mc_sim(N, offset=32, seed=9) as b:
        init = [_np(b.t(i)).copy() for i in ids]
        _abi.check(a.L.lrl_sim_randomize(a.h, *r, C.c_uint32(15), _stream()))
        _abi.check(b.L.lrl_sim_randomize_envs(b.h, C.c_int32(5), C.c_int32(6), *r, C.c_uint32(15), _stream()))
        _abi.check(b.L.lrl_sim_randomize_envs(b.h, C.c_int32(N), C.c_int32(0), *r, C.c_uint32(15), _stream()))
        torch.cuda.synchronize()
        for i, v0 in zip(ids, init):
            ga, gb = _np(a.t(i)), _np(b.t(i))
            same(gb[5:11], ga[5:11], f"tensor {i} inside the range")
            same(gb[:5], v0[:5], f"tensor {i} below the range")
            same(gb[11:], v0[11:], f"tensor {i} above the range")
        for first, cnt in ((-1, 2), (10, 4), (0, N + 1), (3, -1)):
            with pytest.raises(RuntimeError, match="env range"):
                _abi.check(b.L.lrl_sim_randomize_envs(b.h, C.c_int32(first), C.c_int32(cnt), *r, C.c_uint32(15),
                                                      _stream()))


# ---------------------------------------------------------------------------------------------- teleport
TELE = {"terrain.mesh_type": "trimesh", "terrain.teleport_robots": True, "terrain.border_size": 2.0,
        "terrain.terrain_length": 4.0, "terrain.terrain_width": 4.0, "terrain.num_cols": 3,
        "terrain.max_init_terrain_level": 1, "domain_rand.push_robots": False}
TELE_TR = dict(TELE, **{"terrain.teleport_thresh": 0.25, "terrain.num_rows": 4})
TELE_EV = dict(TELE, **{"terrain.teleport_thresh": 0.5, "terrain.num_rows": 3})
ROUGH_TILES = {"terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2], "terrain.terrain_noise_magnitude": 0.05}
TELE_BUILDS = {"plane": ("go1", 6, 7, {}), "mesh_pgs": ("go1", 18, 9, ROUGH_TILES),
               "mesh_tgs": ("go1", 18, 9, dict(ROUGH_TILES, **{"sim.physx.terrain_solver_type": 1}))}


def _teleport_numpy(x, y, t, xo):
    """_teleport_robots (legged_robot.py:768-791) in float32, the four lines in order."""
    x, y = x.copy(), y.copy()
    th, tl, tw = f32(t.teleport_thresh), f32(t.terrain_length), f32(t.terrain_width)
    rows, cols, xo = f32(t.num_rows), f32(t.num_cols), f32(int(xo))
    x[x < th + xo] += tl * (rows - f32(1))
    x[x > tl * rows - th + xo] -= tl * (rows - f32(1))
    y[y < th] += tw * (cols - f32(1))
    y[y > tw * cols - th] -= tw * (cols - f32(1))
    return x, y


@pytest.mark.parametrize("build", list(TELE_BUILDS))
def test_teleport_uses_each_groups_threshold_and_rows(build):
    robot, n_tr, n_ev, extra = TELE_BUILDS[build]
    env = _split(robot, n_tr, dict(TELE_TR, **extra), n_ev, dict(TELE_EV, **extra))
    try:
        assert _build_of(env) == build
        N, G = n_tr + n_ev, env._G
        assert G is not None and (G.teleport_thresh, G.terrain_rows) == (0.5, 3) and env._P.terrain_rows == 4
        root = _np(env.root_states).copy()
        eps = f32(1e-3)
        want_x, want_y = root[:, 0].copy(), root[:, 1].copy()
        moved = np.zeros((N, 2), bool)
        for rows, c in ((np.arange(N) < n_tr, env.cfg), (np.arange(N) >= n_tr, env.eval_cfg)):
            t = c.terrain
            xo = f32(int(t.x_offset * t.horizontal_scale))  # the eval tiles lie below the train tiles
            assert (xo > 0) == bool(rows[-1])
            lo_x, hi_x = f32(t.teleport_thresh) + xo, f32(t.terrain_length * t.num_rows - t.teleport_thresh) + xo
            lo_y, hi_y = f32(t.teleport_thresh), f32(t.terrain_width * t.num_cols - t.teleport_thresh)
            # just outside / inside each of the four thresholds, x and y cases paired per robot
            xs = np.array([lo_x - eps, lo_x + eps, hi_x + eps, hi_x - eps], f32)
            ys = np.array([lo_y + eps, lo_y - eps, hi_y - eps, hi_y + eps], f32)
            k = np.arange(int(rows.sum())) % 4
            root[rows, 0], root[rows, 1] = xs[k], ys[k]
            want_x[rows], want_y[rows] = _teleport_numpy(root[rows, 0], root[rows, 1], t, t.x_offset * t.horizontal_scale)
            moved[rows] = np.stack([want_x[rows] != root[rows, 0], want_y[rows] != root[rows, 1]], 1)
            assert moved[rows][:4].tolist() == [[True, False], [False, True], [True, False], [False, True]]
        # the groups' constants do differ where it matters: the eval rows read with the train group's values would not
        # give these results
        tx, _ = _teleport_numpy(root[n_tr:, 0], root[n_tr:, 1], env.cfg.terrain, 0)
        assert not np.array_equal(tx, want_x[n_tr:])
        env.root_states[:] = _dev(root)
        rng = np.random.default_rng(1)
        act = torch.zeros(N, 12, device="cuda:0")
        noise, dr = _dev(rng.random((N, env._P.num_obs), dtype=f32)), _dev(np.zeros(N, f32))
        _step(env._L, env._sim, env._stream(), act, INJECT, noise, dr)
        out = _np(env.root_states)
        same(out[:, 0], want_x, f"{build} x")
        same(out[:, 1], want_y, f"{build} y")
        same(out[:, 2:], root[:, 2:], f"{build} rest of the root state")
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- eval_group off
@pytest.mark.parametrize("build", ["plane", "mesh_pgs"])
def test_group_forced_on_with_equal_values_changes_nothing(build):
    """A split sim with equal cfgs (no eval block) and the same sim with the eval block switched on and filled with the
    train values: bit-identical state, observations and rewards over 3 physics steps, redraws and pushes included."""
    robot, n_tr, n_ev, base = BUILDS[build]
    over = dict(dict(base, **GROUP_A), **{"domain_rand.push_interval_s": 0.03})  # pushes every 2nd step
    N = n_tr + n_ev
    rng = np.random.default_rng(11)
    acts = [_dev(rng.normal(size=(N, 12)).astype(f32) * 0.3) for _ in range(3)]
    tids = (_abi.T_ROOT_STATE, _abi.T_DOF_POS, _abi.T_DOF_VEL, _abi.T_OBS, _abi.T_PRIV_OBS, _abi.T_REWARD,
            _abi.T_MOTOR_STRENGTH, _abi.T_KP_FACTOR, _abi.T_KD_FACTOR, _abi.T_EPISODE_SUMS, _abi.T_CONTACT_FORCE)
    out = []
    for forced in (False, True):
        env = _split(robot, n_tr, over, n_ev, over, seed=2)
        try:
            assert env._G is None and _build_of(env) == build
            if forced:
                Gf = lparams.group_params(env._P)
                _abi.check(env._L.lrl_sim_set_eval_group(env._sim, C.byref(Gf)))
            env.reset_idx(torch.arange(N, device="cuda:0"))
            env.root_states[:, 2] += 0.34  # (custom origins leave the root at the tile's top: lift it to standing height)
            env.episode_length_buf[:] = _dev(np.array([300, 299, 298, 5, 4])[np.arange(N) % 5], torch.int32)
            run = []
            for a in acts:
                _step(env._L, env._sim, env._stream(), a, _abi.STEP_PHYSICS)
                run.append([_np(env._tensor(i)).copy() for i in tids])
            out.append(run)
        finally:
            env.close()
    for k in range(3):
        for i, a, b in zip(tids, out[0][k], out[1][k]):
            same(b, a, f"{build} step {k} tensor {i}")
    assert not np.array_equal(out[0][0][6], out[0][2][6])  # (motor strengths were redrawn on the way)


# ---------------------------------------------------------------------------------------------- Runner
def test_runner_learns_one_iteration_with_a_differing_eval_cfg():
    from lrl.history import HistoryWrapper
    from lrl.ppo import runner as R
    n_tr, n_ev = 64, 32
    R.RunnerArgs.save_interval = 0
    env = _split("mc", n_tr, {"domain_rand.push_robots": True, "domain_rand.push_interval_s": 0.2}, n_ev,
                 {"domain_rand.push_robots": False, "domain_rand.friction_range": [0.05, 0.06]})
    try:
        assert env._G is not None and env._G.push_robots == 0 and env._P.push_robots == 1
        henv = HistoryWrapper(env)
        runner = R.Runner(henv, device="cuda:0", seed=3)
        runner.learn(1, eval_freq=1)
        assert runner.alg.storage.num_envs == n_tr
        assert "eval/episode" in env.extras
        fr = _np(env.friction_coeffs)
        assert np.all((fr[n_tr:] >= f32(0.05)) & (fr[n_tr:] <= f32(0.06)))
        assert np.sum(fr[:n_tr] > f32(0.06)) > n_tr // 2  # the train envs keep the train range [0.05, 4.5]
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- validation
def test_eval_block_is_validated():
    _, _, M, P = make("mc")
    with mc_sim(8) as s:
        G = lparams.group_params(P)
        G.push_robots, G.push_interval = 1, 0
        with pytest.raises(RuntimeError, match="push_interval"):
            _abi.check(s.L.lrl_sim_set_eval_group(s.h, C.byref(G)))
        G.push_robots = 0  # a group that does not push may carry interval 0
        _abi.check(s.L.lrl_sim_set_eval_group(s.h, C.byref(G)))
        G.push_robots, G.push_interval = 1, 3
        _abi.check(s.L.lrl_sim_set_eval_group(s.h, C.byref(G)))
        # the eval group alone pushes: an injected step needs the push uniforms
        assert P.push_robots == 0
        act = torch.zeros(8, 12, device="cuda:0")
        noise, dr = torch.zeros(8, P.num_obs, device="cuda:0"), torch.zeros(8, device="cuda:0")
        _abi.check(s.L.lrl_sim_inject_uniforms(s.h, C.c_void_p(noise.data_ptr()), C.c_void_p(dr.data_ptr())))
        with pytest.raises(RuntimeError, match="push uniforms"):
            _abi.check(s.L.lrl_sim_step(s.h, C.c_void_p(act.data_ptr()), C.c_uint32(INJECT), _stream()))
        _abi.check(s.L.lrl_sim_set_eval_group(s.h, None))  # off again: the step runs without them
        _abi.check(s.L.lrl_sim_step(s.h, C.c_void_p(act.data_ptr()), C.c_uint32(INJECT), _stream()))
        torch.cuda.synchronize()
