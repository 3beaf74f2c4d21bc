"""The env step kernel's rigid-body dynamics against tests/dyn_ref.py, the FK-only reference that shares nothing with
the kernel or the CPU oracle: one env step of one sub-step (control.decimation = 1) under torque
control, from the input sets of tests/dyn_cases.py, driven as test_env_gpu.py drives the oracle-parity tests.

Free flight: the kernel's (nu+ - nu) / dt is plugged into the reference's 18 equations with the torque the kernel
applied.  Bar per row group (N, N m, N m): 4 x the worst residual of the oracle's float build on the same inputs -
the same operation in another float32 order, this project's habit for the FK bars (test_aux_gpu.py).

Contact (plane under TGS and PGS, the synthetic rough mesh): the rate of the total linear momentum minus m g against
the sum of the kernel's own contact forces, normalised by m |g| + sum_b |F_b| of the float64 oracle; bar 4 x the float
build's worst.  On the plane every body's force points up and lies inside the friction cone.  No env is excluded.

Nothing is taken from the kernel's output to set a bar.  Measured on an MI355X (worst over the envs; the float build's
value x 4 is the bar):

    case                       quantity             float build   bar         kernel
    mc   n=256 free flight     linear (N)           1.462e-03     5.846e-03   1.366e-03
    mc   n=256 free flight     angular (N m)        2.592e-04     1.037e-03   3.341e-04
    mc   n=256 free flight     joint (N m)          1.105e-04     4.421e-04   1.140e-04
    go1  n=256 free flight     linear (N)           2.297e-03     9.189e-03   1.785e-03
    go1  n=256 free flight     angular (N m)        1.464e-04     5.855e-04   2.140e-04
    go1  n=256 free flight     joint (N m)          3.039e-05     1.216e-04   3.188e-05
    mc   n=256 plane TGS       normalised balance   4.790e-06     1.916e-05   5.317e-06
    mc   n=256 plane PGS       normalised balance   4.790e-06     1.916e-05   5.320e-06
    mc   n=256 mesh            normalised balance   4.055e-06     1.622e-05   4.911e-06
    go1  n=256 plane TGS       normalised balance   2.856e-06     1.143e-05   2.681e-06
    go1  n=256 plane PGS       normalised balance   3.080e-06     1.232e-05   2.681e-06
    go1  n=256 mesh            normalised balance   2.617e-06     1.047e-05   2.607e-06

(the n = 37 cases: profiles/dyn_independent_stats.txt).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dyn_cases as dc
from helpers import robot_table
from lrl import _abi
from lrl import config as lcfg
from oracle import oracle
from test_env_gpu import _dev, _env, _np, _step_raw

pytestmark = pytest.mark.gpu

ONE_SUBSTEP = {"control.decimation": 1, "control.control_type": "T"}
MARGIN = 4.0


def _record(line):
    """One JSON line per case to $LRL_DYN_STATS when set (profiles/dyn_independent_stats.txt)."""
    print(json.dumps(line))
    path = os.environ.get("LRL_DYN_STATS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def _rough_env(robot, n, **over):
    """A LeggedRobotEnv on a generated trimesh ground (the tiles of test_terrain_gpu.py; the test replaces the mesh)."""
    from lrl.env import LeggedRobotEnv
    over = dict({"terrain.mesh_type": "trimesh", "terrain.measure_heights": True, "terrain.curriculum": True,
                 "terrain.border_size": dc.MESH_BORDER, "terrain.teleport_robots": False, "terrain.num_rows": 4,
                 "terrain.num_cols": 5, "terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2],
                 "env.num_observations": 42 + 187}, **over)
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    cfg.env.num_envs = n
    for k, v in over.items():
        node = cfg
        *ps, leaf = k.split(".")
        for p in ps:
            node = getattr(node, p)
        setattr(node, leaf, v)
    cfg.terrain.max_init_terrain_level = min(cfg.terrain.max_init_terrain_level, cfg.terrain.num_rows - 1)
    return LeggedRobotEnv("cuda:0", cfg=cfg, seed=5)


def _one_substep(env, P, inp):
    """Writes the input set into the sim, steps once, and returns what the kernel left: (root, qd, contact forces,
    applied torques)."""
    assert env._P.decimation == 1 and env._P.control_type == 2 and not env._P.push_robots
    n = inp["root"].shape[0]
    for attr, key in dict(root_states="root", dof_pos="q", dof_vel="qd", friction_coeffs="friction",
                          restitutions="restitution", payloads="payload", com_displacements="com").items():
        getattr(env, attr)[:] = _dev(inp[key]).reshape(getattr(env, attr).shape)
    env.motor_strengths[:] = 1.0
    rng = np.random.default_rng(n)
    noise, redraw = rng.random((n, env._P.num_obs)).astype(np.float32), rng.random(n).astype(np.float32)
    _step_raw(env, _dev(inp["act"]), _abi.STEP_PHYSICS | _abi.STEP_INJECT_UNIFORM, _dev(noise), _dev(redraw))
    root, qd, con, tau = (_np(getattr(env, a)).copy() for a in ("root_states", "dof_vel", "contact_forces", "torques"))
    assert np.isfinite(root).all() and np.isfinite(qd).all() and np.isfinite(con).all()
    # torque control: the kernel applied what the input set asked for (the CPU records used inp["tau"])
    assert (np.abs(tau) > 1).any()
    np.testing.assert_allclose(tau, inp["tau"], rtol=1e-6, atol=0)
    return root, qd, con, tau


@pytest.mark.parametrize("n", [256, 37])
@pytest.mark.parametrize("robot", ["mc", "go1"])
def test_free_flight_closes_every_equation(robot, n):
    """Base 5 m up, self-collision off: no contact force, and the kernel's acceleration closes the reference's 18
    equations within 4 x the float build's worst residual, per row group."""
    over = dict(ONE_SUBSTEP, **dc.FREE)
    table, M, P = robot_table(robot, **over)
    inp = dc.free_inputs(robot, n)
    env = _env(robot, n, **over)
    assert env._P.self_collisions == 0
    root, qd, con, tau = _one_substep(env, P, inp)
    env.close()
    assert not con.any()
    flt = dc.run_oracle(M, P, inp, library=oracle.cpu_lib(), tau=tau)
    assert (flt[3] == 0).all()
    res = dc.residuals(table, P, inp, {"kernel": (root, qd), "float": flt[:2]}, tau=tau)
    got, ref = dc.by_group(res["kernel"]), dc.by_group(res["float"])
    _record({"case": f"{robot} n={n} free flight", "float_build": ref, "kernel": got, "margin": MARGIN})
    for k in ref:
        assert got[k] <= MARGIN * ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("ground,solver", [("plane", 1), ("plane", 0), ("mesh", 0)])
@pytest.mark.parametrize("n", [256, 37])
@pytest.mark.parametrize("robot", ["mc", "go1"])
def test_contact_forces_balance_the_momentum(robot, n, ground, solver):
    """Standing, tilted, low and penetrating robots on the plane (solver_type 1: TGS, the preset; 0: PGS) and on the
    synthetic mesh handed over through lrl_sim_set_terrain: d/dt p - m g of the kernel's step equals the sum of its
    own contact forces within 4 x the float build's worst normalised error; on the plane the forces respect sign and
    cone.  Every env counts."""
    over = dict(ONE_SUBSTEP, **{"sim.physx.solver_type": solver})
    inp = dc.contact_inputs(robot, n, ground)
    if ground == "plane":
        table, M, P = robot_table(robot, **over)
        env = _env(robot, n, **over)
    else:
        table, M, P = dc.rough_params(robot, **over)
        vtx, samples, world, heights = dc.mesh(float(P.horizontal_scale), float(P.vertical_scale))
        oracle.set_terrain(world, heights)
        oracle.set_terrain(world, heights, library=oracle.cpu_lib())
        env = _rough_env(robot, n, **over)
        assert env._P.terrain_mesh == 1 and env._P.border_size == P.border_size == dc.MESH_BORDER
        assert env._P.horizontal_scale == P.horizontal_scale and env._P.vertical_scale == P.vertical_scale
        _abi.check(_abi.lib().lrl_sim_set_terrain(env._sim, vtx.ctypes.data_as(C.c_void_p),
                                                  samples.ctypes.data_as(C.c_void_p), C.c_int32(dc.MESH_G),
                                                  C.c_int32(dc.MESH_G)))
    assert env._P.solver_tgs == P.solver_tgs == int(solver == 1 and ground == "plane")
    root, qd, con, tau = _one_substep(env, P, inp)
    env.close()
    ref = dc.run_oracle(M, P, inp, tau=tau)
    flt = dc.run_oracle(M, P, inp, library=oracle.cpu_lib(), tau=tau)
    touching = (np.abs(con).sum((1, 2)) > 0).mean()
    assert touching > 0.5 and (ref[3] > 0).mean() > 0.7, (touching, (ref[3] > 0).mean())  # loaded; within the offset
    err = dc.balance_error(table, P, inp, {"kernel": (root, qd, con), "float": flt[:3]}, ref[2])
    _record({"case": f"{robot} n={n} {ground} {'TGS' if P.solver_tgs else 'PGS'}", "float_build": float(err["float"].max()),
             "kernel": float(err["kernel"].max()), "margin": MARGIN, "touching": float(touching),
             "largest_force": float(np.abs(con).max())})
    assert err["kernel"].max() <= MARGIN * err["float"].max(), (err["kernel"].max(), err["float"].max())
    if ground == "plane":
        worst = dc.cone_violation(P, inp, con)
        assert worst.max() <= 0, (np.argmax(worst), worst.max())
