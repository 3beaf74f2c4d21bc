"""The scenes tests/test_depth_ref.py (CPU, the checker alone) and tests/test_depth_gpu.py (the kernel against the
checker) share: the Go1 rough-trimesh cfg of test_render_gpu.py::test_trimesh_go1_image, its terrain rebuilt on the host
as LeggedRobotEnv builds it, and the terrain scenes' base poses (constants of the tests, drawn with LRL_DEPTH_NO_ROBOT).
"""
import numpy as np

from lrl import config as lcfg

TERRAIN_SEED = 3
TERRAIN_ENVS = 4
DEPTH_W, DEPTH_H = 24, 16


def quat_rpy(roll, pitch, yaw):
    """xyzw quaternion of R = Rz(yaw) Ry(pitch) Rx(roll), degrees."""
    r, p, y = (np.deg2rad(a) / 2 for a in (roll, pitch, yaw))
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], np.float32)


def go1_trimesh_cfg(n=TERRAIN_ENVS):
    cfg = lcfg.make_cfg()
    lcfg.config_go1(cfg)
    dr = cfg.domain_rand
    for key in ("push_robots", "randomize_friction", "randomize_restitution", "randomize_motor_strength",
                "randomize_base_mass", "randomize_Kd_factor", "randomize_Kp_factor", "randomize_com_displacement"):
        setattr(dr, key, False)
    cfg.env.num_envs = n
    t = cfg.terrain
    t.num_rows, t.num_cols, t.border_size = 3, 5, 0
    t.mesh_type, t.curriculum, t.teleport_robots = "trimesh", True, False
    t.terrain_proportions = [0.1, 0.1, 0.35, 0.25, 0.2]  # legged_robot_config.py:57
    t.max_init_terrain_level = min(t.max_init_terrain_level, t.num_rows - 1)
    return cfg


def terrain_vertices(cfg, seed=TERRAIN_SEED):
    """The world-frame vertex grid [rows, cols, 3] (float64 of the float32 values lrl_sim_set_terrain places) of the
    terrain LeggedRobotEnv(cfg=cfg, seed=seed) builds: numpy's global RNG seeded with the env seed."""
    from lrl.terrain import Terrain
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        t = Terrain(cfg.terrain, cfg.env.num_envs, None, 0)
    finally:
        np.random.set_state(state)
    rows, cols = t.heightsamples.shape
    vtx = np.array(t.vertices, np.float32).reshape(rows, cols, 3)
    vtx[..., :2] -= np.float32(cfg.terrain.border_size)
    return vtx.astype(np.float64)


# env -> (base position, base rpy in degrees, camera overrides).  The grid spans x in [0, 24], y in [0, 40].
#   0: near the grid's x = 0 edge looking outward (yaw 180): the rays leave the grid
#   1: far = 0.5: most pixels see nothing within it
#   2: camera pitched 45 degrees down
#   3: a rolled and pitched base over the middle of the map
TERRAIN_SCENES = {
    0: dict(pos=(1.2, 20.3, 0.15), rpy=(4.0, -3.0, 180.0), cam=dict()),
    1: dict(pos=(9.1, 13.7, -0.05), rpy=(-6.0, 5.0, 40.0), cam=dict(far=0.5)),
    2: dict(pos=(14.6, 27.2, 0.95), rpy=(8.0, 2.0, -75.0), cam=dict(pitch_deg=45.0)),
    3: dict(pos=(12.3, 6.4, 0.20), rpy=(-12.0, 9.0, 110.0), cam=dict()),
}


def terrain_camera(over):
    cam = dict(pos=(0.27, 0.0, 0.03), pitch_deg=20.0, hfov_deg=87.0, near=0.05, far=3.0, width=DEPTH_W,
               height=DEPTH_H)
    cam.update(over)
    return cam


def reach(cam):
    """The longest ray of the image: rays end at planar distance far, so a corner ray is far sqrt(1 + u^2 + v^2) long."""
    th = np.tan(np.deg2rad(float(cam["hfov_deg"])) / 2)
    return float(cam["far"]) * float(np.sqrt(1 + th * th + (th * cam["height"] / cam["width"]) ** 2))
