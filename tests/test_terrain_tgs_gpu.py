"""The env kernel's terrain-mesh TGS build (Cfg.sim.physx.terrain_solver_type = 1, lrl_env_mesh_tgs.hip) on cuda:0
against the fp64 oracle with its solver switch set (oracle.set_solver_tgs): the setup, bars and caps of
test_terrain_gpu.py::test_rough_terrain_physics_matches_oracle, which checks the PGS build the same way."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import (MAX_EXCLUDED, SEP_EPS_1, VEL_EPS, make_rough, oracle_sensitivity, perturb_state, physics_mismatch,
                     same, sim_of)
from lrl import _abi
from oracle import oracle
from terrain_tgs_common import FLAGS, PARITY, Setup, copy_state, rough_cfg

pytestmark = pytest.mark.gpu

LDS_CAP = 160 * 1024  # the CU's LDS: one 16-env workgroup of the mesh builds


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _step_raw(env, actions, noise, dr):
    L = _abi.lib()
    env._inj = (noise, dr)
    _abi.check(L.lrl_sim_inject_uniforms(env._sim, C.c_void_p(noise.data_ptr()), C.c_void_p(dr.data_ptr())))
    _abi.check(L.lrl_sim_step(env._sim, C.c_void_p(actions.data_ptr()), C.c_uint32(FLAGS), env._stream()))
    torch.cuda.synchronize()


def _got(env):
    return {k: _np(getattr(env, a)) for k, a in dict(root="root_states", dof_pos="dof_pos", dof_vel="dof_vel",
                                                      contact="contact_forces", h="measured_heights").items()}


def _load(env, st, fr, rs):
    env.root_states[:] = _dev(st["root"])
    env.dof_pos[:] = _dev(st["dof_pos"])
    env.dof_vel[:] = _dev(st["dof_vel"])
    env.friction_coeffs[:] = _dev(fr)
    env.restitutions[:] = _dev(rs)
    env.payloads[:] = 0.0
    env.com_displacements[:] = 0.0


@functools.lru_cache(None)
def _parity_run(robot, n, steps, env_seed, pose_seed, perturb_seed, with_pgs, above=(0.25, 0.40, 0.12)):
    """`steps` steps of the opted-in env, re-synchronised to the TGS oracle's state before each; per step the GPU's
    arrays, the oracle's, its discontinuity margins and its sensitive envs.  with_pgs: also, for step 1, the PGS
    oracle's result from the same start with its margins and sensitive envs.  Computed once per argument set."""
    from lrl.env import LeggedRobotEnv
    over = PARITY["over"]
    env = LeggedRobotEnv("cuda:0", cfg=rough_cfg(n, robot, **over), seed=env_seed)
    try:
        assert env._P.terrain_mesh == 1 and np.abs(env.terrain.heightsamples).max() > 0
        assert env._P.solver_tgs == 1 and env.solver == "tgs"
        S = Setup(robot, n, over, env_seed, pose_seed, perturb_seed, terrain=env.terrain, above=above)
        out = []
        for s in range(steps):
            _load(env, S.st, S.fr, S.rs)
            act, noise, dr = S.draws()
            _step_raw(env, _dev(act), _dev(noise), _dev(dr))
            rec = {}
            if with_pgs and s == 0:
                rng_q = np.random.default_rng(perturb_seed + 1)
                st0 = copy_state(S.st)
                st_a, st_b, st_c = copy_state(st0), perturb_state(st0, rng_q), perturb_state(st0, rng_q)
                mg = np.zeros((n, 2))
                S.oracle_step(st_a, act, noise, dr, 1, False, mg)
                S.oracle_step(st_b, act, noise, dr, 1, False)
                S.oracle_step(st_c, act, noise, dr, 1, False)
                rec["pgs"] = (st_a, mg, oracle_sensitivity(st_a, st_b) | oracle_sensitivity(st_a, st_c))
            margins, sens, st_p = S.oracle_step_with_sensitivity(act, noise, dr, s + 1)
            rec.update(got=_got(env), st=copy_state(S.st), margins=margins, sens=sens)
            out.append(rec)
        return S.P, out
    finally:
        env.close()


def _check_parity(tag, P, recs, heights=True):
    touched = 0.0
    for s, r in enumerate(recs):
        got, st, margins, sens = r["got"], r["st"], r["margins"], r["sens"]
        n = len(sens)
        touched = max(touched, (np.abs(st["contact"]).sum((1, 2)) > 0).mean())
        bad, excl = physics_mismatch(got, st, margins, sens, sep_eps=SEP_EPS_1)
        print(f"{tag} n={n} step {s + 1}/{len(recs)}: {excl.sum()} envs excluded ({excl.mean():.3f}; discontinuity margin "
              f"{((margins[:, 0] < SEP_EPS_1) | (margins[:, 1] < VEL_EPS)).sum()}, oracle-sensitive {sens.sum()}), "
              f"{bad.sum()} outside tolerance, touching {touched:.2f}")
        for e in np.flatnonzero(bad)[:4]:  # diagnostics of a failure
            print(e, "margins", margins[e], "root", got["root"][e] - st["root"][e],
                  "dq", got["dof_pos"][e] - st["dof_pos"][e])
        assert bad.sum() == 0, (s, np.flatnonzero(bad)[:16])
        assert excl.mean() <= MAX_EXCLUDED, (s, excl.mean())
        assert np.isfinite(got["root"]).all() and np.isfinite(got["dof_vel"]).all()
        if heights:  # the height scan of the GPU's own final pose through the oracle: bit-exact
            ref_h = np.stack([np.array([oracle.height_sample(P, q, k) for q in got["root"]], np.float32)
                              for k in range(P.num_height_points)], 1)
            np.testing.assert_array_equal(got["h"], ref_h)
    assert touched > 0.5, touched  # the poses do touch the terrain


@pytest.mark.parametrize("steps", [1, 10])
def test_mesh_tgs_matches_oracle(steps):
    """Go1 on stairs, slopes, obstacles and stepping stones with the key set against the oracle's TGS on the same mesh,
    1 and 10 steps re-synchronised to the oracle's state before each: zero envs outside helpers.TOL, at most
    MAX_EXCLUDED on a discontinuity, more than half touching the mesh; the height scan bit-exact."""
    P, recs = _parity_run("go1", PARITY["n"], steps, PARITY["env_seed"], PARITY["pose_seed"], PARITY["perturb_seed"],
                          steps == 1)
    _check_parity("terrain tgs", P, recs)


def test_mesh_tgs_is_not_pgs():
    """The same opted-in one-step GPU result against the oracle's PGS: more than a quarter of the envs outside the bars
    (the kernel really runs another solver than the default build)."""
    _, recs = _parity_run("go1", PARITY["n"], 1, PARITY["env_seed"], PARITY["pose_seed"], PARITY["perturb_seed"], True)
    st, margins, sens = recs[0]["pgs"]
    bad, excl = physics_mismatch(recs[0]["got"], st, margins, sens, sep_eps=SEP_EPS_1)
    print(f"opted-in GPU step vs the PGS oracle: {bad.mean():.3f} of the envs outside the bars, {excl.mean():.3f} excluded")
    assert bad.mean() > 0.25, bad.mean()


def test_mini_cheetah_mesh_tgs_matches_oracle():
    """Mini Cheetah (hull support tables, 28-sphere rows) on the non-flat curriculum trimesh, 64 envs, one step, the
    same bars.  Seeds: env 5, poses 9, perturbations 78 as for the Go1, the bases 0.18-0.30 m above the local terrain
    top and a quarter at 0.08 m (the smaller robot stands lower: at the Go1's heights only 31 % of the envs touch the
    mesh).  The oracle alone under TGS excludes 1 of the 64 envs on these inputs, with 75 % touching (measured on the
    CPU)."""
    P, recs = _parity_run("mc", 64, 1, PARITY["env_seed"], PARITY["pose_seed"], PARITY["perturb_seed"], False,
                          (0.18, 0.30, 0.08))
    _check_parity("terrain tgs mc", P, recs)


def test_key_without_tgs_runs_the_pgs_build_unchanged():
    """terrain_solver_type = 1 with solver_type = 0 is PGS: root, dof, contact and obs arrays bit-identical to an env
    without the key after 3 steps of the same injected draws."""
    from lrl.env import LeggedRobotEnv
    n, over = 64, PARITY["over"]
    res = []
    for key in (True, False):
        cfg = rough_cfg(n, "go1", terrain_solver_type=1 if key else None, **over)
        if key:
            cfg.sim.physx.solver_type = 0
        env = LeggedRobotEnv("cuda:0", cfg=cfg, seed=PARITY["env_seed"])
        try:
            assert env._P.terrain_mesh == 1 and env._P.solver_tgs == 0 and env.solver == "pgs"
            S = Setup("go1", n, over, PARITY["env_seed"], PARITY["pose_seed"], PARITY["perturb_seed"],
                      terrain=env.terrain)
            _load(env, S.st, S.fr, S.rs)
            for _ in range(3):
                act, noise, dr = S.draws()
                _step_raw(env, _dev(act), _dev(noise), _dev(dr))
            res.append(dict(_got(env), obs=_np(env.obs_buf)))
        finally:
            env.close()
    assert np.abs(res[0]["contact"]).sum() > 0
    for k in ("root", "dof_pos", "dof_vel", "contact", "obs"):
        same(res[0][k], res[1][k], k)


def test_eval_cfg_with_another_terrain_solver_is_refused():
    """The train / eval split shares one kernel parameter block: an eval cfg that differs from the train cfg in the
    key (so in solver_tgs) is refused like any other per-step kernel parameter."""
    from lrl.env import LeggedRobotEnv
    over = PARITY["over"]
    with pytest.raises(NotImplementedError, match="solver_tgs"):
        LeggedRobotEnv("cuda:0", cfg=rough_cfg(48, "go1", **over),
                       eval_cfg=rough_cfg(16, "go1", terrain_solver_type=None, **over), seed=PARITY["env_seed"])


def test_standing_on_the_tiles_stays_sane():
    """64 Go1 standing (zero actions) on the curriculum tiles for 200 steps with the key set: all finite, every base
    within 5 cm of its height at step 50, projected gravity z < -0.9 (upright).  The robots are set down on the
    platforms of their tiles (stairs up and down, slopes, obstacles: 16 each over 6 levels, the platforms between 1.4 m
    below and 1.8 m above zero), at the default pose with the feet on the local ground, random yaw and up to 0.5 m off
    the tile centre; the env's own start poses drop them from the tile origin's height, up to a metre above the ground
    of the downward tiles, where they tumble and reset under either solver."""
    from lrl.env import LeggedRobotEnv
    n = 64
    cfg = rough_cfg(n, "go1", **{"terrain.num_rows": 6, "terrain.num_cols": 4, "terrain.border_size": 3.0,
                                 "noise.add_noise": False, "domain_rand.randomize_com_displacement": False,
                                 "domain_rand.randomize_base_mass": False})
    env = LeggedRobotEnv("cuda:0", cfg=cfg, seed=1)
    try:
        assert env.solver == "tgs" and env._P.terrain_mesh == 1
        env.reset()
        tc = cfg.terrain
        hs = env.terrain.heightsamples.astype(np.float32) * np.float32(tc.vertical_scale)
        rng = np.random.default_rng(3)
        root = np.zeros((n, 13), np.float32)
        root[:, :2] = _np(env.env_origins)[:, :2] + rng.uniform(-0.5, 0.5, (n, 2))
        ix = ((root[:, 0] + tc.border_size) / tc.horizontal_scale).astype(int)
        iy = ((root[:, 1] + tc.border_size) / tc.horizontal_scale).astype(int)
        ground = np.array([hs[i - 5:i + 6, j - 5:j + 6].max() for i, j in zip(ix, iy)], np.float32)
        root[:, 2] = ground + np.float32(cfg.init_state.pos[2])
        yaw = rng.uniform(-np.pi, np.pi, n)
        root[:, 5], root[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
        env.root_states[:] = _dev(root)
        env.dof_pos[:] = _dev(np.tile(np.array(env._P.default_dof_pos[:], np.float32), (n, 1)))
        env.dof_vel[:] = 0.0
        assert ground.max() - ground.min() > 1.0  # the tiles' platforms are at different heights
        zero = torch.zeros(n, 12, device="cuda:0")
        z50 = None
        for i in range(200):
            env.step(zero)
            if i == 49:
                z50 = _np(env.root_states)[:, 2].copy()
        torch.cuda.synchronize()
        root1, pg = _np(env.root_states), _np(env.projected_gravity)
        assert np.isfinite(root1).all() and np.isfinite(_np(env.dof_vel)).all() and np.isfinite(_np(env.obs_buf)).all()
        dz = np.abs(root1[:, 2] - z50)
        print(f"standing 200 steps: largest base height change since step 50 {dz.max():.4f} m, largest projected "
              f"gravity z {pg[:, 2].max():.4f}, base above the local ground {np.sort(root1[:, 2] - ground)[[0, -1]]}")
        assert np.abs(_np(env.contact_forces)).sum() > 0  # standing on the mesh
        assert dz.max() < 0.05, np.sort(dz)[-8:]
        assert pg[:, 2].max() < -0.9, np.sort(pg[:, 2])[-8:]
    finally:
        env.close()


@pytest.mark.parametrize("robot", ["go1", "mc"])
def test_mesh_tgs_lds_fits(robot):
    """Both presets create a terrain-mesh TGS sim at 16 envs per wave: the LDS of the build it launches is within the
    CU's, and above the PGS build's by the twelve dz leg fields (the restitution targets live in dead query scratch)."""
    _, _, M, P1 = make_rough(robot, **{"sim.physx.terrain_solver_type": 1})
    _, _, _, P0 = make_rough(robot)
    assert P1.terrain_mesh == 1 and P1.solver_tgs == 1 and P0.solver_tgs == 0
    L = _abi.lib()
    with sim_of(M, P1, 64) as s1, sim_of(M, P0, 64) as s0:
        tgs, pgs = L.lrl_debug_sim_lds_bytes(s1.h), L.lrl_debug_sim_lds_bytes(s0.h)
    print(f"{robot}: mesh TGS build {tgs} B of LDS, mesh PGS build {pgs} B")
    assert 0 < pgs < tgs <= LDS_CAP, (pgs, tgs)
    assert tgs - pgs == 12 * 16 * 4, (pgs, tgs)
