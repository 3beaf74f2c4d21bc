"""Shared by test_obs_layouts.py / test_obs_layouts_gpu.py: the fixture cases of tests/golden/make_golden_obs.py and a
numpy float32 restatement of the observation row (legged_robot.py:342-389) from an env's own post-step tensors."""
import numpy as np

ALL_ON = {"env.observe_vel": True, "env.observe_only_ang_vel": True, "env.observe_only_lin_vel": True,
          "env.observe_yaw": True, "commands.global_reference": True, "noise.add_noise": False}
# case -> (robot, fixture, cfg overrides)  (make_golden_obs.py CASES)
CASES = {
    "lin": ("mc", "post_physics_obs_lin.npz", {"env.observe_only_lin_vel": True, "env.num_observations": 45}),
    "ang": ("mc", "post_physics_obs_ang.npz",
            {"env.observe_only_ang_vel": True, "noise.add_noise": False, "env.num_observations": 45}),
    "yaw_global": ("go1", "post_physics_obs_yaw_global.npz",
                   {"env.observe_vel": True, "env.observe_yaw": True, "commands.global_reference": True,
                    "env.num_observations": 49}),
    "all": ("go1", "post_physics_obs_all.npz", dict(ALL_ON, **{"env.num_observations": 55})),
}
SWITCHES = {"observe_only_ang_vel": "env.observe_only_ang_vel", "observe_only_lin_vel": "env.observe_only_lin_vel",
            "observe_yaw": "env.observe_yaw", "global_reference": "commands.global_reference"}

F = np.float32
TWO_PI, PI = F(2 * np.pi), F(np.pi)


def heading64(quat):
    """atan2 of the rotated x axis in float64 (for the wrap-margin conditions)."""
    x, y, z, w = np.asarray(quat, np.float64).T
    return np.arctan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))


def yaw_entry(quat):
    """clip(0.5 * wrap_to_pi(atan2(forward.y, forward.x)), -1, 1), forward = quat_apply(quat, [1, 0, 0]) with
    torch_utils' operation order, every step rounded to float32."""
    x, y, z, w = (np.asarray(quat, F)[:, k] for k in range(4))
    zero, one, two = F(0), F(1), F(2)
    t0, t1, t2 = (y * zero - z * zero) * two, (z * one - x * zero) * two, (x * zero - y * one) * two
    fx = (one + w * t0) + (y * t2 - z * t1)
    fy = (zero + w * t1) + (z * t0 - x * t2)
    a = np.arctan2(fy, fx).astype(F)
    a = np.where(a < 0, a + TWO_PI, a).astype(F)  # python-style remainder by float32(2 pi) of a value in [-pi, pi]
    a = np.where(a > PI, a - TWO_PI, a).astype(F)
    return np.clip(F(0.5) * a, F(-1), F(1)).astype(F)


def expected_rows(env, cfg):
    """The rows compute_observations builds from ``env``'s current tensors, without noise, clipped at
    clip_observations: numpy float32, one operation per rounding."""
    g = lambda t: t.detach().cpu().numpy().astype(F)
    s = cfg.normalization.obs_scales
    root, blv, bav = g(env.root_states), g(env.base_lin_vel), g(env.base_ang_vel)
    parts = [g(env.projected_gravity)]
    if cfg.env.observe_command:
        parts.append(g(env.commands)[:, :3] * np.array([s.lin_vel, s.lin_vel, s.ang_vel], F))
    parts += [(g(env.dof_pos) - g(env.default_dof_pos)) * F(s.dof_pos), g(env.dof_vel) * F(s.dof_vel), g(env.actions)]
    if cfg.env.observe_vel:
        lin = root[:, 7:10] if cfg.commands.global_reference else blv
        parts = [lin * F(s.lin_vel), bav * F(s.ang_vel)] + parts
    if cfg.env.observe_only_ang_vel:
        parts = [bav * F(s.ang_vel)] + parts
    if cfg.env.observe_only_lin_vel:
        parts = [blv * F(s.lin_vel)] + parts
    if cfg.env.observe_yaw:
        parts.append(yaw_entry(root[:, 3:7])[:, None])
    if cfg.terrain.measure_heights:
        h = np.clip(root[:, 2:3] - F(0.5) - g(env.measured_heights), F(-1), F(1)) * F(s.height_measurements)
        parts.append(h.astype(F))
    row = np.concatenate(parts, axis=1).astype(F)
    c = F(cfg.normalization.clip_observations)
    return np.clip(row, -c, c)
