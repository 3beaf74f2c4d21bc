"""Environment / training configuration tree with the reference's attribute paths.

Mirrors the surface of ``Cfg`` (mini_gym/envs/base/legged_robot_config.py:6-256) and the robot
presets ``config_mini_cheetah`` (mini_gym/envs/mini_cheetah/mini_cheetah_config.py:8-105) and
``config_go1`` (mini_gym/envs/go1/go1_config.py:8-107): the same section names, field names and
values, so that code written against ``Cfg.env.num_envs`` / ``vars(Cfg.rewards.scales)`` keeps
working.  The tree is built from plain dict specs into ``Section`` namespaces (no params_proto):
``vars(section)`` returns fields in declaration order, which fixes the reward-term order
(legged_robot.py:1079-1093).
"""
import copy
import types
import weakref

ROOT = None  # filled by lrl/__init__.py: directory holding resources/


_PATHS = {}  # id(Section) -> (weak ref, its dotted path in the tree: "terrain", "rewards.scales"), for _update's prefixes


def _update_fields(obj, names, own_paths, d=None, **kwargs):
    """params_proto's ``_update(deps)`` (scripts/play.py:30-44 restores a run's parameters with it): every key of
    ``d`` / ``kwargs`` that names a field of ``obj`` — plainly (``mesh_type``) or under the node's own prefix
    (``terrain.mesh_type``, ``Cfg.terrain.mesh_type``) — sets it; other keys are left for the other nodes."""
    items = dict(d or {}, **kwargs)
    for k, v in items.items():
        prefix, _, leaf = str(k).rpartition(".")
        if leaf not in names:
            continue
        if prefix and not any(prefix == p or prefix.endswith("." + p) for p in own_paths):
            continue
        setattr(obj, leaf, copy.deepcopy(v))


class ArgsProto:
    """Base of the algorithm argument classes (AC_Args, PPO_Args, RunnerArgs): ``Cls._update(dict)`` as params_proto's
    PrefixProto, keys plain or prefixed with the class name."""

    @classmethod
    def _update(cls, d=None, **kwargs):
        _update_fields(cls, {k for k in vars(cls) if not k.startswith("_")}, (cls.__name__,), d, **kwargs)


class Section(types.SimpleNamespace):
    """A config node; attribute access like the reference's PrefixProto classes."""

    def _update(self, d=None, **kwargs):
        ref, path = _PATHS.get(id(self), (None, None))
        path = path if ref is not None and ref() is self else None
        _update_fields(self, set(vars(self)), (path,) if path else (), d, **kwargs)

    def to_dict(self):
        out = {}
        for k, v in vars(self).items():
            out[k] = v.to_dict() if isinstance(v, Section) else copy.deepcopy(v)
        return out


def _build(spec, path=""):
    sec = Section()
    if path:
        _PATHS[id(sec)] = (weakref.ref(sec), path)
    for k, v in spec.items():
        setattr(sec, k, _build(v, f"{path}.{k}" if path else k)
                if isinstance(v, dict) and not k.endswith(("_angles", "stiffness", "damping")) else copy.deepcopy(v))
    return sec


# Base defaults (legged_robot_config.py:7-256), field order preserved.
_BASE = {
    "env": dict(num_envs=4096, num_observations=235, num_privileged_obs=18, privileged_future_horizon=1,
                num_actions=12, num_observation_history=15, env_spacing=3.0, send_timeouts=True,
                episode_length_s=20, observe_vel=True, observe_only_ang_vel=False, observe_only_lin_vel=False,
                observe_yaw=False, observe_command=True, record_video=True, priv_observe_friction=True,
                priv_observe_restitution=True, priv_observe_base_mass=True, priv_observe_com_displacement=True,
                priv_observe_motor_strength=True, priv_observe_Kp_factor=True, priv_observe_Kd_factor=True),
    "terrain": dict(mesh_type="trimesh", horizontal_scale=0.1, vertical_scale=0.005, border_size=0,
                    curriculum=True, static_friction=1.0, dynamic_friction=1.0, restitution=0.0,
                    terrain_noise_magnitude=0.1, terrain_smoothness=0.005, measure_heights=True,
                    measured_points_x=[round(-0.8 + 0.1 * i, 1) for i in range(17)],
                    measured_points_y=[round(-0.5 + 0.1 * i, 1) for i in range(11)],
                    selected=False, terrain_kwargs=None, min_init_terrain_level=0, max_init_terrain_level=5,
                    terrain_length=8.0, terrain_width=8.0, num_rows=10, num_cols=20,
                    terrain_proportions=[0.1, 0.1, 0.35, 0.25, 0.2], slope_treshold=0.75, difficulty_scale=1.0,
                    x_init_range=1.0, y_init_range=1.0, x_init_offset=0.0, y_init_offset=0.0,
                    teleport_robots=True, teleport_thresh=2.0, max_platform_height=0.2),
    "commands": dict(command_curriculum=False, max_reverse_curriculum=1.0, max_forward_curriculum=1.0,
                     forward_curriculum_threshold=0.8, yaw_command_curriculum=False, max_yaw_curriculum=1.0,
                     yaw_curriculum_threshold=0.5, num_commands=4, resampling_time=10.0, heading_command=True,
                     global_reference=False, num_lin_vel_bins=20, lin_vel_step=0.3, num_ang_vel_bins=20,
                     ang_vel_step=0.3, distribution_update_extension_distance=1, curriculum_seed=100,
                     lin_vel_x=[-1.0, 1.0], lin_vel_y=[-1.0, 1.0], ang_vel_yaw=[-1, 1],
                     body_height_cmd=[-0.05, 0.05], impulse_height_commands=False,
                     limit_vel_x=[-10.0, 10.0], limit_vel_y=[-0.6, 0.6], limit_vel_yaw=[-10.0, 10.0],
                     heading=[-3.14, 3.14]),
    "init_state": dict(pos=[0.0, 0.0, 1.0], rot=[0.0, 0.0, 0.0, 1.0], lin_vel=[0.0, 0.0, 0.0],
                       ang_vel=[0.0, 0.0, 0.0], default_joint_angles={"joint_a": 0.0, "joint_b": 0.0}),
    "control": dict(control_type="P", stiffness={"joint_a": 10.0, "joint_b": 15.0},
                    damping={"joint_a": 1.0, "joint_b": 1.5}, action_scale=0.5, hip_scale_reduction=1.0,
                    decimation=4),
    "asset": dict(file="", foot_name="None", penalize_contacts_on=[], terminate_after_contacts_on=[],
                  disable_gravity=False, collapse_fixed_joints=True, fix_base_link=False,
                  default_dof_drive_mode=3, self_collisions=0, replace_cylinder_with_capsule=True,
                  flip_visual_attachments=True, density=0.001, angular_damping=0.0, linear_damping=0.0,
                  max_angular_velocity=1000.0, max_linear_velocity=1000.0, armature=0.0, thickness=0.01),
    "domain_rand": dict(rand_interval_s=10, randomize_friction=True, friction_range=[0.5, 1.25],
                        randomize_restitution=False, restitution_range=[0, 1.0], randomize_base_mass=False,
                        added_mass_range=[-1.0, 1.0], randomize_com_displacement=False,
                        com_displacement_range=[-0.15, 0.15], randomize_motor_strength=False,
                        motor_strength_range=[0.9, 1.1], randomize_Kp_factor=False, Kp_factor_range=[0.8, 1.3],
                        randomize_Kd_factor=False, Kd_factor_range=[0.5, 1.5], push_robots=True,
                        push_interval_s=15, max_push_vel_xy=1.0),
    "rewards": dict(only_positive_rewards=True, tracking_sigma=0.25, tracking_sigma_lat=0.25,
                    tracking_sigma_long=0.25, tracking_sigma_yaw=0.25, soft_dof_pos_limit=1.0,
                    soft_dof_vel_limit=1.0, soft_torque_limit=1.0, base_height_target=1.0, max_contact_force=100.0,
                    use_terminal_body_height=False, terminal_body_height=0.20,
                    scales=dict(termination=-0.0, tracking_lin_vel=1.0, tracking_ang_vel=0.5, lin_vel_z=-2.0,
                                ang_vel_xy=-0.05, orientation=-0.0, torques=-0.00001, dof_vel=-0.0,
                                dof_acc=-2.5e-7, base_height=-0.0, feet_air_time=1.0, collision=-1.0,
                                feet_stumble=-0.0, action_rate=-0.01, stand_still=-0.0, tracking_lin_vel_lat=0.0,
                                tracking_lin_vel_long=0.0)),
    "normalization": dict(obs_scales=dict(lin_vel=2.0, ang_vel=0.25, dof_pos=1.0, dof_vel=0.05,
                                          height_measurements=5.0, body_height_cmd=2.0),
                          clip_observations=100.0, clip_actions=100.0, friction_range=[0.05, 4.5],
                          restitution_range=[0, 1.0], added_mass_range=[-1.0, 3.0],
                          com_displacement_range=[-0.1, 0.1], motor_strength_range=[0.9, 1.1],
                          Kp_factor_range=[0.8, 1.3], Kd_factor_range=[0.5, 1.5]),
    "noise": dict(add_noise=True, noise_level=1.0,
                  noise_scales=dict(dof_pos=0.01, dof_vel=1.5, lin_vel=0.1, ang_vel=0.2, gravity=0.05,
                                    height_measurements=0.1)),
    "viewer": dict(ref_env=0, pos=[-10, 0, 6], lookat=[0.0, 0, 3.0]),
    "sim": dict(dt=0.005, substeps=1, gravity=[0.0, 0.0, -9.81], up_axis=1, use_gpu_pipeline=True,
                physx=dict(num_threads=10, solver_type=1, num_position_iterations=4, num_velocity_iterations=0,
                           contact_offset=0.01, rest_offset=0.0, bounce_threshold_velocity=0.5,
                           max_depenetration_velocity=1.0, max_gpu_contact_pairs=2 ** 23,
                           default_buffer_size_multiplier=5, contact_collection=2)),
}


def make_cfg():
    """A fresh, independent base configuration tree."""
    return _build(_BASE)


Cfg = make_cfg()

# The egocentric depth camera's group (project-only: the reference has no such sensor, so the defaults above do not
# hold it and vars(Cfg) / to_dict() are the reference's; add_depth_camera installs it).
_DEPTH = dict(width=64, height=48, hfov_deg=87.0, pos=[0.27, 0.0, 0.03], pitch_deg=20.0, near=0.05, far=3.0,
              update_interval=5, see_robot=True)


def add_depth_camera(cfg, **overrides):
    """Install ``cfg.depth``: every env of a ``LeggedRobotEnv`` built from ``cfg`` then carries a depth camera bolted
    to its base (``env.depth_images``, lrl_sim_depth).  Fields: ``width`` x ``height`` pixels, ``hfov_deg``, the mount
    point ``pos`` in the base frame, ``pitch_deg`` about the base's y axis (positive looks down), the ``near`` / ``far``
    clamps in metres, ``update_interval`` (env steps between full refreshes; an env that was reset is redrawn at once)
    and ``see_robot`` (False: the env's own body is not drawn).

    The defaults are choices modelled on a trunk-mounted RealSense-class sensor read at 10 Hz (64 x 48 after
    downsampling, 87 degree horizontal field of view, a 3 m working range, every 5th 50 Hz policy step); they are not
    measurements of any robot or camera.  ``overrides`` replace them; an unknown key is an error."""
    unknown = set(overrides) - set(_DEPTH)
    if unknown:
        raise KeyError(f"add_depth_camera: unknown field(s) {sorted(unknown)}; known: {', '.join(_DEPTH)}")
    cfg.depth = _build(dict(_DEPTH, **overrides), "depth")
    return cfg


# The depth sensor model's group (project-only, a group of its own: Cfg.depth keeps its nine keys).
_DEPTH_SENSOR = dict(noise_a=0.001, noise_b=0.005, dropout_p=0.01, edge_thresh=0.1, invalid_value=None, quant=0.001,
                     latency_frames=[0, 1])


def add_depth_sensor(cfg, **overrides):
    """Install ``cfg.depth_sensor``: a ``LeggedRobotEnv`` built from ``cfg`` (which also needs ``cfg.depth``,
    add_depth_camera) then keeps ``env.depth_sensed`` beside the exact ``env.depth_images``: what a stereo depth camera
    would deliver of them (lrl_sim_depth_sense, include/lrl.h states the model).  Fields: the range noise's standard
    deviation ``noise_a + noise_b z^2`` in metres, ``dropout_p`` (share of pixels lost at random), ``edge_thresh``
    (relative depth step to a 4-neighbour at which both sides are lost; 0: none), ``invalid_value`` (what a lost pixel
    reads; None: the camera's ``far``), ``quant`` (range step in metres; 0: none) and ``latency_frames`` = [min, max]:
    each episode draws a delay from it, counted in the camera's full refreshes.

    The defaults are choices in the range data sheets of RealSense-class stereo cameras give (millimetre noise at
    arm's length growing with the square of the range, about a percent of holes, one refresh of delay at most); they
    are not measurements of any camera.  ``overrides`` replace them; an unknown key is an error."""
    unknown = set(overrides) - set(_DEPTH_SENSOR)
    if unknown:
        raise KeyError(f"add_depth_sensor: unknown field(s) {sorted(unknown)}; known: {', '.join(_DEPTH_SENSOR)}")
    vals = dict(_DEPTH_SENSOR, **overrides)
    vals["latency_frames"] = list(vals["latency_frames"])
    cfg.depth_sensor = _build(vals, "depth_sensor")
    return cfg

_LEG_ORDER = ("FL", "RL", "FR", "RR")


def _angles(hip, thigh, calf):
    d = {}
    for part, vals in (("hip", hip), ("thigh", thigh), ("calf", calf)):
        for leg, v in zip(_LEG_ORDER, vals):
            d[f"{leg}_{part}_joint"] = v
    return d


def _apply(cfg, updates):
    for path, value in updates.items():
        node = cfg
        *parents, leaf = path.split(".")
        for p in parents:
            node = getattr(node, p)
        setattr(node, leaf, copy.deepcopy(value))


def _register_paths(sec, path=""):
    if path:
        _PATHS[id(sec)] = (weakref.ref(sec), path)
    for k, v in vars(sec).items():
        if isinstance(v, Section):
            _register_paths(v, f"{path}.{k}" if path else k)


def _dr_preset(friction, restitution, added_mass, com, motor_strength):
    """One evaluation preset of the domain randomisation: the five ranges that differ between the presets; the switches,
    the (unused) Kp / Kd ranges and the push settings are the same in all of them."""
    return {
        "domain_rand.randomize_friction": True, "domain_rand.friction_range": friction,
        "domain_rand.randomize_restitution": True, "domain_rand.restitution_range": restitution,
        "domain_rand.restitution": 0.5,
        "domain_rand.randomize_base_mass": True, "domain_rand.added_mass_range": added_mass,
        "domain_rand.randomize_com_displacement": True, "domain_rand.com_displacement_range": com,
        "domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": motor_strength,
        "domain_rand.randomize_Kp_factor": False, "domain_rand.Kp_factor_range": [0.8, 1.3],
        "domain_rand.randomize_Kd_factor": False, "domain_rand.Kd_factor_range": [0.5, 1.5],
        "domain_rand.push_robots": False, "domain_rand.push_interval_s": 15, "domain_rand.max_push_vel_xy": 1.0,
    }


# Evaluation presets: cfg path -> value, the settings of the reference's mini_gym_learn/eval_metrics/
# domain_randomization.py (DR_SETTINGS and base_set; tests/golden/dr_settings.json holds what its functions assign).
# The six DR presets touch only what an eval group may change (lrl/params.py GROUP_FIELDS and the rigid-body
# draws at creation), so each one works as an eval_cfg beside a training cfg.  "base_set" does not: the episode length
# and the terminal body height are per-step kernel parameters shared by both groups, so it is for a stand-alone
# evaluation env (scripts/evaluate.py), and as an eval_cfg lrl.params.eval_group_params refuses it.
EVAL_PRESETS = {
    "base_set": {
        "terrain.teleport_robots": True, "terrain.border_size": 50, "terrain.num_rows": 10, "terrain.num_cols": 10,
        "commands.resampling_time": 1e9, "env.episode_length_s": 500,
        "rewards.terminal_body_height": 0.0, "rewards.use_terminal_body_height": True,
    },
    "rand_regular": _dr_preset([0.05, 4.5], [0, 1.0], [-1.0, 3.0], [-0.1, 0.1], [0.9, 1.1]),
    "rand_large": _dr_preset([0.04, 6.0], [0, 1.0], [-1.5, 4.0], [-0.13, 0.13], [0.88, 1.12]),
    # motor_strength_range [0.9, -0.99] is the reference's value (by the other presets' pattern [0.9, 0.91] was
    # meant): kept, so the motor strengths are drawn from (-0.99, 0.9], sign changes included
    "static_low": _dr_preset([0.05, 0.06], [0, 0.01], [-1.0, -0.99], [-0.1, -0.09], [0.9, -0.99]),
    "static_medium": _dr_preset([1.0, 1.01], [0.5, 0.51], [0.0, 0.01], [0.0, 0.01], [1.0, 1.01]),
    "static_high": _dr_preset([4.49, 4.5], [0.99, 1.0], [2.99, 3.0], [0.09, 0.1], [1.09, 1.1]),
    "only_base_mass": _dr_preset([1.0, 1.01], [0.5, 0.51], [-1, 3], [0.0, 0.01], [1.0, 1.01]),
}
DR_PRESETS = tuple(k for k in EVAL_PRESETS if k != "base_set")


def preset_sets(name):
    """A preset as ``--eval-set`` strings (``PATH=VALUE``, the value's python literal)."""
    if name not in EVAL_PRESETS:
        raise KeyError(f"unknown evaluation preset {name!r}; known: {', '.join(EVAL_PRESETS)}")
    return [f"{path}={value!r}" for path, value in EVAL_PRESETS[name].items()]


def eval_variant(cfg, num_envs, sets=(), preset=None):
    """An eval cfg for ``LeggedRobotEnv(cfg=cfg, eval_cfg=...)``: an independent copy of ``cfg`` with ``num_envs`` envs
    and the assignments ``sets`` applied, each a string ``PATH=VALUE`` (scripts/train.py --eval-set) whose value is a
    python literal: ``domain_rand.friction_range=[0.05,0.06]``, ``domain_rand.push_robots=True``.  PATH must name an
    existing field (a typo would otherwise evaluate on the training distribution without a word).

    ``preset``: the name of an ``EVAL_PRESETS`` entry (or several, applied in order) set before ``sets``, so an explicit
    set overrides it.  The DR presets give a valid eval_cfg; ``base_set`` changes per-step kernel parameters (episode
    length, terminal body height) and therefore only suits a stand-alone evaluation env, whose cfg the result then is."""
    import ast
    ecfg = copy.deepcopy(cfg)
    _register_paths(ecfg)
    ecfg.env.num_envs = int(num_envs)
    for name in ((preset,) if isinstance(preset, str) else tuple(preset or ())):
        if name not in EVAL_PRESETS:
            raise KeyError(f"unknown evaluation preset {name!r}; known: {', '.join(EVAL_PRESETS)}")
        _apply(ecfg, EVAL_PRESETS[name])  # (may add domain_rand.restitution, as the robot presets do)
    for item in sets:
        path, sep, text = str(item).partition("=")
        if not sep:
            raise ValueError(f"--eval-set wants PATH=VALUE, got {item!r}")
        node = ecfg
        *parents, leaf = path.strip().split(".")
        for p in parents:
            node = getattr(node, p)
        if not hasattr(node, leaf):
            raise AttributeError(f"cfg has no field {path.strip()!r}")
        setattr(node, leaf, ast.literal_eval(text.strip()))
    return ecfg


_COMMON_PRESET = {
    "control.control_type": "P", "control.stiffness": {"joint": 20.0}, "control.damping": {"joint": 0.5},
    "control.action_scale": 0.25, "control.hip_scale_reduction": 0.5, "control.decimation": 4,
    "asset.self_collisions": 0, "asset.flip_visual_attachments": False, "asset.fix_base_link": False,
    "rewards.soft_dof_pos_limit": 0.9, "rewards.scales.dof_pos_limits": -10.0,
    "rewards.scales.orientation": -5.0, "rewards.scales.base_height": -30.0,
    "terrain.measure_heights": False, "terrain.terrain_noise_magnitude": 0.0, "terrain.border_size": 50,
    "terrain.terrain_proportions": [0, 0, 0, 0, 0, 0, 0, 0, 1.0], "terrain.curriculum": False,
    "env.num_observations": 42, "env.observe_vel": False,
    "commands.heading_command": False, "commands.resampling_time": 10.0, "commands.command_curriculum": True,
    "commands.num_lin_vel_bins": 30, "commands.num_ang_vel_bins": 30, "commands.lin_vel_x": [-0.6, 0.6],
    "commands.lin_vel_y": [-0.6, 0.6], "commands.ang_vel_yaw": [-1, 1],
    "domain_rand.randomize_base_mass": True, "domain_rand.added_mass_range": [-1, 3],
    "domain_rand.push_robots": False, "domain_rand.max_push_vel_xy": 0.5, "domain_rand.randomize_friction": True,
    "domain_rand.friction_range": [0.05, 4.5], "domain_rand.randomize_restitution": True,
    "domain_rand.restitution_range": [0.0, 1.0], "domain_rand.restitution": 0.5,
    "domain_rand.randomize_com_displacement": True, "domain_rand.com_displacement_range": [-0.1, 0.1],
    "domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": [0.9, 1.1],
    "domain_rand.randomize_Kp_factor": False, "domain_rand.Kp_factor_range": [0.8, 1.3],
    "domain_rand.randomize_Kd_factor": False, "domain_rand.Kd_factor_range": [0.5, 1.5],
    "domain_rand.rand_interval_s": 6,
}


def config_mini_cheetah(cfg):
    """Mini Cheetah preset (mini_cheetah_config.py:8-105)."""
    upd = dict(_COMMON_PRESET)
    upd.update({
        "init_state.pos": [0.0, 0.0, 0.32],
        "init_state.default_joint_angles": _angles((0.1, 0.1, -0.1, -0.1), (-0.8,) * 4, (1.62,) * 4),
        "asset.file": "{MINI_GYM_ROOT_DIR}/resources/robots/mini_cheetah/urdf/mini_cheetah.urdf",
        "asset.foot_name": "calf", "asset.penalize_contacts_on": [],
        "asset.terminate_after_contacts_on": ["base", "thigh"],
        "rewards.base_height_target": 0.30, "rewards.scales.torques": -0.0002,
        "terrain.mesh_type": "trimesh", "terrain.teleport_robots": True, "env.num_envs": 4000,
    })
    _apply(cfg, upd)
    # keep the reference's declaration order: torques/orientation/base_height were already
    # declared in the base tree; dof_pos_limits is new and lands last (legged_robot.py:1079).
    return cfg


def config_go1(cfg):
    """Unitree Go1 preset (go1_config.py:8-107)."""
    upd = dict(_COMMON_PRESET)
    upd.update({
        "init_state.pos": [0.0, 0.0, 0.34],
        "init_state.default_joint_angles": _angles((0.1, 0.1, -0.1, -0.1), (0.8, 1.0, 0.8, 1.0), (-1.5,) * 4),
        "asset.file": "{MINI_GYM_ROOT_DIR}/resources/robots/go1/urdf/go1.urdf",
        "asset.foot_name": "foot", "asset.penalize_contacts_on": ["thigh", "calf"],
        "asset.terminate_after_contacts_on": ["base"],
        "rewards.base_height_target": 0.34, "rewards.scales.torques": -0.0001,
        "rewards.scales.action_rate": -0.01,
        "terrain.mesh_type": "plane", "terrain.teleport_robots": False, "env.num_envs": 4096,
    })
    _apply(cfg, upd)
    return cfg
