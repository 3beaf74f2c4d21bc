"""The terrain-mesh solver switch (Cfg.sim.physx.terrain_solver_type, build_params(terrain_solver_type=)) on the host,
and the yardstick of tests/test_terrain_tgs_gpu.py: on that test's inputs the oracle's TGS and PGS are different
solvers, so a kernel that matched one cannot match the other."""
import numpy as np

from helpers import TOL, make_rough, within_tolerance
from lrl import params as lparams
from terrain_tgs_common import PARITY, Setup, copy_state


def _fields(P):
    return {f: (bytes(getattr(P, f)) if hasattr(getattr(P, f), "_length_") else getattr(P, f))
            for f, _ in type(P)._fields_}


def test_switch_follows_key_and_keyword():
    cfg, rob, _, P = make_rough("go1")
    assert cfg.sim.physx.solver_type == 1 and not hasattr(cfg.sim.physx, "terrain_solver_type")
    assert P.terrain_mesh == 1 and P.solver_tgs == 0  # the default did not move
    bp = lambda c=cfg, **kw: lparams.build_params(c, rob, terrain_mesh=1, **kw)
    assert bp().solver_tgs == 0
    assert bp(terrain_solver_type=0).solver_tgs == 0
    assert bp(terrain_solver_type=1).solver_tgs == 1
    assert bp(terrain_solver_type=1, solver_type=0).solver_tgs == 0
    # the cfg key says what the keyword says, and the keyword overrides it
    cfg1, _, _, P1 = make_rough("go1", **{"sim.physx.terrain_solver_type": 1})
    assert P1.solver_tgs == 1
    assert _fields(P1) == _fields(bp(terrain_solver_type=1))
    assert bp(cfg1, terrain_solver_type=0).solver_tgs == 0
    assert bp(cfg1, solver_type=0).solver_tgs == 0
    cfg0, _, _, P0 = make_rough("go1", **{"sim.physx.terrain_solver_type": 0})
    assert _fields(P0) == _fields(P)
    # nothing else in the parameter block moves with it
    a, b = _fields(P), _fields(P1)
    assert [f for f in a if a[f] != b[f]] == ["solver_tgs"]
    # the defaults (cfg dumps, script-surface fixtures) do not carry the key
    from lrl import config as lcfg
    assert "terrain_solver_type" not in lcfg.make_cfg().sim.physx.to_dict()


def test_key_changes_nothing_on_the_plane():
    for robot in ("go1", "mc"):
        cfg, rob, _, _ = make_rough(robot)
        base = _fields(lparams.build_params(cfg, rob, terrain_mesh=0))
        assert base["solver_tgs"] == 1
        assert _fields(lparams.build_params(cfg, rob, terrain_mesh=0, terrain_solver_type=1)) == base
        assert _fields(lparams.build_params(cfg, rob, terrain_mesh=0, terrain_solver_type=0)) == base
        cfg.sim.physx.terrain_solver_type = 1
        assert _fields(lparams.build_params(cfg, rob, terrain_mesh=0)) == base


def test_oracle_tgs_and_pgs_differ_on_the_parity_inputs():
    """The oracle alone on the GPU parity test's setup: after step 1 more than a quarter of the envs have a PGS result
    outside helpers.TOL of the TGS result (measured: see the printed share), so the GPU test's zero-outside-tolerance
    bar against the TGS oracle cannot be met by a kernel that solves with PGS."""
    S = Setup("go1", PARITY["n"], PARITY["over"], PARITY["env_seed"], PARITY["pose_seed"], PARITY["perturb_seed"])
    act, noise, dr = S.draws()
    st_tgs, st_pgs = copy_state(S.st), copy_state(S.st)
    S.oracle_step(st_tgs, act, noise, dr, 1, tgs=True)
    S.oracle_step(st_pgs, act, noise, dr, 1, tgs=False)
    touched = (np.abs(st_tgs["contact"]).sum((1, 2)) > 0).mean()
    outside = (~within_tolerance(st_pgs, st_tgs, TOL)).mean()
    dqd = np.abs(st_pgs["dof_vel"] - st_tgs["dof_vel"]).max()
    print(f"oracle PGS vs TGS after step 1: {outside:.3f} of the envs outside TOL, largest joint-rate difference "
          f"{dqd:.2f} rad/s, {touched:.2f} of the envs touching the mesh")
    assert touched > 0.5, touched
    assert outside > 0.25, outside
