"""What tests/test_terrain_tgs.py (CPU, the oracle alone) and tests/test_terrain_tgs_gpu.py (the env kernel's
terrain-mesh TGS build against the oracle) share: the rough-terrain cfg with Cfg.sim.physx.terrain_solver_type set, the
terrain the env generates from its seed (built on the host, so the CPU test sees the GPU test's mesh), the poses on it,
and the oracle's steps with its process-global solver switch set around them and restored."""
import contextlib

import numpy as np

from helpers import make_rough, oracle_sensitivity, perturb_state
from lrl import _abi
from lrl import config as lcfg
from lrl import terrain as T
from oracle import oracle

# the parity setup: the shape of test_terrain_gpu.py::test_rough_terrain_physics_matches_oracle
PARITY = dict(n=256, over={"terrain.num_rows": 4, "terrain.num_cols": 5, "terrain.border_size": 3.0}, env_seed=5,
              pose_seed=9, perturb_seed=78)
FLAGS = _abi.STEP_PHYSICS | _abi.STEP_INJECT_UNIFORM


def rough_cfg(n, robot="go1", terrain_solver_type=1, **over):
    """test_terrain_gpu.py's rough cfg (trimesh curriculum tiles, height scan) with the project-only solver key."""
    over = dict({"terrain.mesh_type": "trimesh", "terrain.measure_heights": True, "terrain.curriculum": True,
                 "terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2],  # legged_robot_config.py:57
                 "terrain.border_size": 2.0, "terrain.teleport_robots": False,
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
    if terrain_solver_type is not None:
        cfg.sim.physx.terrain_solver_type = terrain_solver_type
    return cfg


def host_terrain(cfg, n, seed):
    """The map LeggedRobotEnv(cfg, num_envs=n, seed=seed) generates (LeggedRobotEnv._create_terrain)."""
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        return T.Terrain(cfg.terrain, n, None, 0)
    finally:
        np.random.set_state(state)


def oracle_terrain(terrain, tc):
    rows, cols = terrain.heightsamples.shape
    v = terrain.vertices.reshape(rows, cols, 3).copy()
    v[..., :2] -= np.float32(tc.border_size)
    oracle.set_terrain(v, terrain.heightsamples.astype(np.float32) * np.float32(tc.vertical_scale))


def poses_on_terrain(rng, terrain, tc, n, P, above=(0.25, 0.40, 0.12)):
    """test_terrain_gpu.py::_poses_on_terrain: bases 0.25-0.40 m above the local terrain top over the curriculum tiles,
    tilted and moving; a quarter dropped low so links touch the ground.  above: that range and the low height (the
    Go1's; a smaller robot stands lower)."""
    hs = terrain.heightsamples.astype(np.float32) * np.float32(tc.vertical_scale)
    root = np.zeros((n, 13), np.float32)
    root[:, 0] = rng.uniform(0.5, tc.num_rows * tc.terrain_length - 0.5, n)
    root[:, 1] = rng.uniform(0.5, tc.num_cols * tc.terrain_width - 0.5, n)
    ix = ((root[:, 0] + tc.border_size) / tc.horizontal_scale).astype(int)
    iy = ((root[:, 1] + tc.border_size) / tc.horizontal_scale).astype(int)
    top = np.array([hs[max(i - 3, 0):i + 4, max(j - 3, 0):j + 4].max() for i, j in zip(ix, iy)], np.float32)
    root[:, 2] = top + rng.uniform(above[0], above[1], n)
    k = n // 4
    root[:k, 2] = top[:k] + above[2]
    ang = rng.normal(size=(n, 3)) * 0.15
    ang[:, 2] = rng.uniform(-np.pi, np.pi, n)
    th = np.linalg.norm(ang, axis=1, keepdims=True)
    root[:, 3:7] = np.concatenate([ang / np.maximum(th, 1e-9) * np.sin(th / 2), np.cos(th / 2)], 1)
    root[:, 7:10] = rng.normal(size=(n, 3)) * 0.3
    root[:, 10:13] = rng.normal(size=(n, 3)) * 0.5
    dof = np.array(P.default_dof_pos[:], np.float32)[None] + rng.normal(size=(n, 12)).astype(np.float32) * 0.2
    dofv = rng.normal(size=(n, 12)).astype(np.float32)
    return root, dof, dofv


@contextlib.contextmanager
def oracle_solver(tgs):
    """The oracle's solver switch (process-global) set for the block and back at 0 after it."""
    oracle.set_solver_tgs(1 if tgs else 0)
    try:
        yield
    finally:
        oracle.set_solver_tgs(0)


class Setup:
    """Model, opted-in params, the oracle's start state and the rngs of one parity run; `terrain` is the env's own map
    when there is an env, else the host-generated one."""

    def __init__(self, robot, n, over, env_seed, pose_seed, perturb_seed, terrain=None, above=(0.25, 0.40, 0.12)):
        self.n = n
        self.cfg = rough_cfg(n, robot, **over)
        self.terrain = terrain if terrain is not None else host_terrain(self.cfg, n, env_seed)
        _, _, self.M, self.P = make_rough(robot, **over, **{"sim.physx.terrain_solver_type": 1})
        assert self.P.terrain_mesh == 1 and self.P.solver_tgs == 1
        oracle_terrain(self.terrain, self.cfg.terrain)
        self.rng = np.random.default_rng(pose_seed)
        self.rng_p = np.random.default_rng(perturb_seed)
        M, P = self.M, self.P
        root, dof, dofv = poses_on_terrain(self.rng, self.terrain, self.cfg.terrain, n, P, above)
        self.st = oracle.make_state(n, M.num_bodies, P.num_obs, P.num_history, P.num_sum_keys + 1, P.num_sum_keys + 5,
                                    num_height_points=P.num_height_points)
        self.fr = self.rng.uniform(0.05, 4.5, n).astype(np.float32)
        self.rs = self.rng.uniform(0, 1, n).astype(np.float32)
        for k, v in dict(root=root, dof_pos=dof, dof_vel=dofv, friction=self.fr, restitution=self.rs).items():
            self.st[k][:] = v

    def draws(self):
        """The step's actions and injected uniforms (in the order the PGS parity test draws them)."""
        act = (self.rng.normal(size=(self.n, 12)) * 0.5).astype(np.float32)
        noise = self.rng.random((self.n, self.P.num_obs)).astype(np.float32)
        return act, noise, np.full(self.n, np.nan, np.float32)

    def oracle_step(self, st, act, noise, dr, counter, tgs, margins=None):
        with oracle_solver(tgs):
            oracle.env_step(self.M, self.P, st, act, FLAGS, noise_u=noise, dr_u=dr, margins=margins,
                            common_step_counter=counter)

    def oracle_step_with_sensitivity(self, act, noise, dr, counter, tgs=True):
        """Advance self.st one step; returns (margins, the envs whose fp64 result moves out of the bars under two
        fp32-size perturbations of the start state, one perturbed result)."""
        margins = np.zeros((self.n, 2))
        st_p, st_q = perturb_state(self.st, self.rng_p), perturb_state(self.st, self.rng_p)
        self.oracle_step(self.st, act, noise, dr, counter, tgs, margins)
        self.oracle_step(st_p, act, noise, dr, counter, tgs)
        self.oracle_step(st_q, act, noise, dr, counter, tgs)
        return margins, oracle_sensitivity(self.st, st_p) | oracle_sensitivity(self.st, st_q), st_p


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}
