"""ctypes mirror of include/lrl.h (structs, enums) and the loader for liblrl.so.

The product path goes through liblrl.so only: if the library is missing or no GPU is visible the
env / PPO entry points raise instead of falling back to any CPU or eager implementation.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# LRL_LIB overrides the library path (instrumented development builds); the default is the in-tree build
LIB_PATH = os.environ.get("LRL_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "liblrl.so")

MAX_BODIES, MAX_SPHERES, NUM_DOF, NUM_LEGS, MAX_OBS, MAX_REWARD_TERMS, NUM_PRIV = 20, 40, 12, 4, 256, 24, 18
MAX_HEIGHT_POINTS = 192
f32, i32, u32 = C.c_float, C.c_int32, C.c_uint32

REWARD_TERMS = ["lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "energy",
                "energy_expenditure", "dof_vel", "dof_acc", "action_rate", "collision", "survival",
                "dof_pos_limits", "dof_vel_limits", "torque_limits", "tracking_lin_vel", "tracking_ang_vel",
                "feet_air_time", "stumble", "stand_still", "feet_contact_forces"]

STEP_PHYSICS, STEP_HISTORY, STEP_INJECT_UNIFORM = 1, 2, 4

(T_ROOT_STATE, T_DOF_POS, T_DOF_VEL, T_CONTACT_FORCE, T_RIGID_BODY_STATE, T_TORQUES, T_ACTIONS, T_LAST_ACTIONS,
 T_LAST_DOF_VEL, T_LAST_ROOT_VEL, T_COMMANDS, T_OBS, T_PRIV_OBS, T_OBS_HISTORY, T_REWARD, T_RESET, T_TIME_OUT,
 T_EPISODE_LENGTH, T_EPISODE_SUMS, T_COMMAND_SUMS, T_FEET_AIR_TIME, T_LAST_CONTACTS, T_FRICTION, T_RESTITUTION,
 T_PAYLOAD, T_COM_DISPLACEMENT, T_MOTOR_STRENGTH, T_KP_FACTOR, T_KD_FACTOR, T_ENV_ORIGINS, T_BASE_LIN_VEL,
 T_BASE_ANG_VEL, T_PROJECTED_GRAVITY, T_JOINT_POS_TARGET, T_MEASURED_HEIGHTS, T_NUM) = range(36)


class LrlModel(C.Structure):
    _fields_ = [
        ("num_bodies", i32), ("body_leg", i32 * MAX_BODIES), ("body_link", i32 * MAX_BODIES),
        ("joint_xyz", f32 * 3 * 3 * NUM_LEGS), ("joint_quat", f32 * 4 * 3 * NUM_LEGS),
        ("joint_axis", f32 * 3 * 3 * NUM_LEGS), ("foot_xyz", f32 * 3 * NUM_LEGS),
        ("base_mass", f32), ("base_com", f32 * 3), ("base_inertia", f32 * 6),
        ("link_mass", f32 * 3 * NUM_LEGS), ("link_com", f32 * 3 * 3 * NUM_LEGS),
        ("link_inertia", f32 * 6 * 3 * NUM_LEGS),
        ("num_spheres", i32), ("sphere_body", i32 * MAX_SPHERES), ("sphere_pos", f32 * 3 * MAX_SPHERES),
        ("sphere_radius", f32 * MAX_SPHERES),
        ("dof_lower", f32 * NUM_DOF), ("dof_upper", f32 * NUM_DOF), ("dof_effort", f32 * NUM_DOF),
        ("dof_velocity", f32 * NUM_DOF),
        ("sphere_hull", i32 * MAX_SPHERES), ("num_hulls", i32), ("hull_res", i32), ("hull_k", i32),
        ("hull_table", C.c_void_p),
    ]


class LrlGroupParams(C.Structure):
    """lrl_group_params (lrl_sim_set_eval_group): the eval group's own domain-randomisation, push and teleport values;
    every field has the name and type of its LrlEnvParams counterpart."""
    _fields_ = [
        ("randomize_motor_strength", i32), ("randomize_kp", i32), ("randomize_kd", i32),
        ("motor_strength_range", f32 * 2), ("kp_range", f32 * 2), ("kd_range", f32 * 2), ("dr_span", f32 * 3),
        ("push_robots", i32), ("push_interval", i32), ("push_lo", f32), ("push_span", f32),
        ("teleport", i32), ("teleport_thresh", f32), ("terrain_length", f32), ("terrain_width", f32),
        ("terrain_rows", i32), ("terrain_cols", i32),
    ]


class LrlEnvParams(C.Structure):
    _fields_ = [
        ("sim_dt", f32), ("decimation", i32), ("dt", f32), ("gravity", f32 * 3),
        ("contact_offset", f32), ("max_depenetration_velocity", f32), ("bounce_threshold_velocity", f32),
        ("ground_friction", f32), ("ground_restitution", f32), ("solver_iterations", i32), ("baumgarte", f32),
        ("control_type", i32), ("action_scale", f32), ("hip_scale_reduction", f32), ("clip_actions", f32),
        ("p_gains", f32 * NUM_DOF), ("d_gains", f32 * NUM_DOF), ("default_dof_pos", f32 * NUM_DOF),
        ("torque_limits", f32 * NUM_DOF), ("soft_dof_pos_lower", f32 * NUM_DOF),
        ("soft_dof_pos_upper", f32 * NUM_DOF), ("dof_vel_limits", f32 * NUM_DOF),
        ("num_feet", i32), ("feet", i32 * NUM_LEGS), ("termination_mask", u32), ("penalised_mask", u32),
        ("num_reward_terms", i32), ("reward_term", i32 * MAX_REWARD_TERMS), ("reward_scale", f32 * MAX_REWARD_TERMS),
        ("reward_slot", i32 * MAX_REWARD_TERMS), ("num_sum_keys", i32), ("termination_scale", f32),
        ("termination_slot", i32), ("only_positive_rewards", i32),
        ("tracking_sigma", f32), ("tracking_sigma_yaw", f32), ("base_height_target", f32),
        ("soft_dof_vel_limit", f32), ("soft_torque_limit", f32), ("max_contact_force", f32),
        ("use_terminal_body_height", i32), ("terminal_body_height", f32),
        ("num_obs", i32), ("observe_vel", i32), ("observe_command", i32),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32),
        ("obs_scale_dof_vel", f32), ("commands_scale", f32 * 3), ("add_noise", i32), ("noise_vec", f32 * MAX_OBS),
        ("clip_obs", f32), ("priv_scale", f32 * 5), ("priv_shift", f32 * 5),
        ("rand_interval", i32), ("randomize_motor_strength", i32), ("randomize_kp", i32), ("randomize_kd", i32),
        ("motor_strength_range", f32 * 2), ("kp_range", f32 * 2), ("kd_range", f32 * 2),
        ("teleport", i32), ("teleport_thresh", f32), ("teleport_x_offset", f32), ("terrain_length", f32),
        ("terrain_width", f32), ("terrain_rows", i32), ("terrain_cols", i32),
        ("base_init_state", f32 * 13), ("num_history", i32), ("auto_reset", i32), ("max_episode_length", i32),
        ("terrain_mesh", i32), ("border_size", f32), ("horizontal_scale", f32), ("vertical_scale", f32),
        ("measure_heights", i32), ("num_height_points", i32), ("height_points", f32 * 2 * MAX_HEIGHT_POINTS),
        ("obs_scale_height", f32), ("num_train_envs", i32), ("teleport_x_offset_eval", f32), ("dr_span", f32 * 3),
        ("joint_limits", i32), ("joint_limit_margin", f32), ("self_collisions", i32),
        ("push_robots", i32), ("push_interval", i32), ("push_lo", f32), ("push_span", f32),
        ("solver_tgs", i32),
        ("observe_only_ang_vel", i32), ("observe_only_lin_vel", i32), ("observe_yaw", i32), ("global_reference", i32),
    ]


class LrlTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("dtype", i32), ("ndim", i32), ("shape", C.c_int64 * 4),
                ("strides", C.c_int64 * 4)]


# enum lrl_metric (lrl_sim_metrics_*): the named rows in id order, then the internal row of the tables
METRIC_NAMES = ("lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques",
                "power_consumption", "CoT", "froude_number", "termination")
METRIC_NUM = len(METRIC_NAMES)
METRIC_SPEED_XY = METRIC_NUM
METRIC_ROWS = METRIC_NUM + 1
METRICS_REDUCE_DOUBLES = 3 * METRIC_ROWS + 4


class LrlMetricsView(C.Structure):
    """lrl_metrics_view (lrl_sim_metrics_tensors)."""
    _fields_ = [(k, C.c_void_p) for k in ("step", "sum", "sumsq", "max", "steps", "episodes", "falls")] + \
               [("rows", i32), ("named_rows", i32), ("num_envs", i32), ("pitch", C.c_int64)]


class LrlRolloutStore(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("priv", C.c_void_p), ("hist", C.c_void_p), ("actions", C.c_void_p),
                ("values", C.c_void_p), ("logp", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p),
                ("hist_dim", i32), ("hist_ld", i32)]


i64 = C.c_int64


class LrlPpoNet(C.Structure):
    _fields_ = [(k, i32) for k in ("num_obs", "num_priv", "num_hist", "num_actions", "enc_h0", "enc_h1", "latent",
                                    "ac_h0", "ac_h1", "ac_h2", "ad_h0", "ad_h1")] + \
               [(k, i64) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w4a", "b4a", "w4c", "b4c", "e1w", "e1b", "e2w",
                                    "e2b", "e3w", "e3b", "d1w", "d1b", "d2w", "d2b", "d3w", "d3b", "std_off",
                                    "main_begin", "main_end", "adapt_begin", "adapt_end", "kl_slot", "total")] + \
               [("activation", i32), ("plain", i32)]  # 0 = ELU / 1 = tanh; 1 = plain MLP over obs (lrl/hlp)


class LrlPpoBatch(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "priv", "hist", "actions", "values", "returns", "logp", "adv", "mu",
                                          "sigma", "rows")] + [("batch", i32), ("hist_ld", i32)]


class LrlPpoHparams(C.Structure):
    _fields_ = [("clip_param", f32), ("entropy_coef", f32), ("value_loss_coef", f32), ("max_grad_norm", f32),
                ("desired_kl", f32), ("use_clipped_value_loss", i32), ("adaptive_schedule", i32), ("beta1", f32),
                ("beta2", f32), ("eps", f32)]


class LrlDevCurriculum(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("weights", "cdf", "state", "mt_key", "ep_rew_lin", "ep_rew_ang", "env_bins",
                                          "env_bins_f", "command_area", "axes")] + \
               [("half", C.c_double * 3), ("nx", i32), ("ny", i32), ("nz", i32), ("words", C.c_void_p),
                ("draws", C.c_void_p), ("env_bins_f_prev", C.c_void_p), ("command_area_prev", C.c_void_p)]


# enum lrl_nav_term (include/lrl.h): the navigation wrapper's reward names in id order
NAV_TERMS = ("distance", "action_rate", "lateral_vel", "backward_vel", "terminal_distance_covered",
             "terminal_distance_gs", "terminal_ll_reset", "terminal_time_out")
NAV_ONLY_FLAGS, NAV_ONLY_RESET = 0x100, 0x200
NAV_BLOCK = 256  # LRL_NAV_BLOCK


class LrlNavState(C.Structure):
    """lrl_nav_state (lrl_nav_begin_step / lrl_nav_end_step): the navigation wrapper's buffers and scalars."""
    _fields_ = [(k, C.c_void_p) for k in ("obs_buf", "rew_buf", "reset_buf", "gs_buf", "time_buf", "episode_length_buf",
                                          "actions", "last_actions", "last_pos", "dist_travelled", "lateral_vel",
                                          "backward_vel", "goal_position", "episode_sums", "episode_sums_eval", "ids",
                                          "count", "block_counts", "means_train", "means_eval", "means_ll",
                                          "prev_train", "prev_eval", "prev_ll")] + \
               [(k, i32) for k in ("n", "num_train_envs", "max_episode_length", "num_step_terms",
                                   "num_terminal_terms")] + \
               [("base_init_state", f32 * 3), ("term", i32 * MAX_REWARD_TERMS), ("scale", f32 * MAX_REWARD_TERMS),
                ("command_threshold", f32), ("goal_threshold", f32)]


class LrlGemmDesc(C.Structure):
    """lrl_gemm_desc (lrl_gemm_f32_ex): a product in the update's grouped / pitched operand forms."""
    _fields_ = [(k, i32) for k in ("layout", "epi", "M", "N", "K", "groups", "planes", "splits")] + \
               [(k, C.c_void_p) for k in ("A", "B", "C", "bias", "aux", "rows", "workspace")] + \
               [(k, i64) for k in ("lda", "ldb", "ldc", "ld_aux", "ga", "gb", "gc", "gbias", "gaux",
                                    "workspace_floats")] + \
               [("path_out", C.POINTER(i32)), ("splits_out", C.POINTER(i32))]


GEMM_MULTI_NOT_ELIGIBLE = 1  # lrl_gemm_f32_multi: the descriptors are not a set it offers, nothing was launched

# family ids of the path report (LRL_GEMM_PATH_* of include/lrl.h): report = family | bm << 8 | bn << 16 | interior << 24
GEMM_FAMILIES = {1: "x6p", 2: "x6t", 3: "x6", 4: "x6d", 5: "glds", 6: "glds32", 7: "glds_tn", 8: "thin16",
                 9: "thin32", 10: "staged"}


class LrlCamera(C.Structure):
    """lrl_camera (lrl_sim_render / lrl_sim_record)."""
    _fields_ = [("pos", f32 * 3), ("target", f32 * 3), ("hfov_deg", f32), ("far", f32), ("width", i32),
                ("height", i32), ("flags", u32)]


# the camera's constants (the LRL_RENDER_* / LRL_CAM_* defines of include/lrl.h; tests/test_render_abi.py compares)
CAM_FOLLOW = 1
RENDER_ID_SHADOW = 0x10000
RENDER_LINK_RADIUS = 0.02
RENDER_LIGHT = (0.35, -0.45, 0.82)  # towards the light, normalised by its users
RENDER_AMBIENT = 0.35
RENDER_SKY = (0.55, 0.70, 0.90)
RENDER_GROUND_A = (0.80, 0.80, 0.78)
RENDER_GROUND_B = (0.45, 0.47, 0.50)
RENDER_BASE = (0.85, 0.30, 0.20)
RENDER_SPHERE = (0.95, 0.75, 0.15)
RENDER_LINK = (0.20, 0.35, 0.80)


class LrlDepthCamera(C.Structure):
    """lrl_depth_camera (lrl_sim_depth): the base-mounted depth camera every env carries."""
    _fields_ = [("pos", f32 * 3), ("pitch_deg", f32), ("hfov_deg", f32), ("near", f32), ("far", f32), ("width", i32),
                ("height", i32), ("flags", u32)]


# the LRL_DEPTH_* defines of include/lrl.h (tests/test_depth_abi.py compares)
DEPTH_NO_ROBOT = 1


class LrlDepthSensor(C.Structure):
    """lrl_depth_sensor (lrl_sim_depth_sense): the sensor model applied to the exact depth image."""
    _fields_ = [("width", i32), ("height", i32), ("near", f32), ("far", f32), ("noise_a", f32), ("noise_b", f32),
                ("dropout_p", f32), ("edge_thresh", f32), ("invalid_value", f32), ("quant", f32),
                ("latency_min", i32), ("latency_max", i32)]


# the LRL_SENSE_* enum of include/lrl.h (lrl_sim_depth_sense's mode; tests/test_depth_sensor_abi.py compares)
SENSE_PUSH, SENSE_RESET_ONLY, SENSE_FILL = 0, 1, 2
RNG_DEPTH = 8  # LRL_RNG_DEPTH (include/lrl_philox.h): the sensor's Philox stream


PPO_CTRL_BYTES = 64  # sizeof(lrl_ppo_ctrl): double lr, double loss_sum[3], float mb[4], float x4


def fill(struct, **kw):
    """Assign python values (scalars / nested lists) into a ctypes struct."""
    for k, v in kw.items():
        cur = getattr(struct, k)
        if isinstance(cur, C.Array):
            _fill_array(cur, v)
        else:
            setattr(struct, k, v)
    return struct


def _fill_array(arr, v):
    for i, x in enumerate(v):
        if isinstance(arr[i], C.Array):
            _fill_array(arr[i], x)
        else:
            arr[i] = x


_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "lrl.h")
# the depth sensor model's part of the ABI: a header of its own that lrl.h includes (lrl_sim_depth_sense)
_SENSE_HEADER = os.path.join(os.path.dirname(_HEADER), "lrl_depth_sense.h")
# the history shift done by the rollout act, likewise (lrl_ppo_act_shift, lrl_sim_history_preshifted)
_SHIFT_HEADER = os.path.join(os.path.dirname(_HEADER), "lrl_history_shift.h")


def source_hash():
    """sha256 (first 16 hex digits) of the sources liblrl.so must have been built from: the files of csrc/Makefile's
    SRCS then HDRS, the order of its SRC_HASH (the Makefile is one of them: other build flags make a stale library)."""
    import hashlib
    with open(os.path.join(_CSRC, "Makefile")) as f:
        mk = f.read()
    h = hashlib.sha256()
    for var in ("SRCS", "HDRS"):
        for name in re.search(rf"^{var} = (.*)$", mk, re.M).group(1).split():
            with open(os.path.join(_CSRC, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


# the structs of include/lrl.h this module mirrors: a pointer to one of them is POINTER(mirror) in a signature
MIRRORS = {"lrl_model": LrlModel, "lrl_env_params": LrlEnvParams, "lrl_group_params": LrlGroupParams,
           "lrl_tensor": LrlTensor, "lrl_metrics_view": LrlMetricsView, "lrl_rollout_store": LrlRolloutStore,
           "lrl_ppo_net": LrlPpoNet, "lrl_ppo_batch": LrlPpoBatch, "lrl_ppo_hparams": LrlPpoHparams,
           "lrl_dev_curriculum": LrlDevCurriculum, "lrl_nav_state": LrlNavState, "lrl_gemm_desc": LrlGemmDesc,
           "lrl_camera": LrlCamera, "lrl_depth_camera": LrlDepthCamera}
# (lrl_depth_sensor, like lrl_vision_net, is not among them: its entry point takes byref(LrlDepthSensor) as a plain
# pointer; tests/test_depth_sensor_abi.py compares its layout with the header's)
_SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_RETURNS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "const char*": C.c_char_p}


def signatures(header):
    """{name: (restype, argtypes)} of every lrl_* prototype in the text of a header.  The header is the ABI: scalars
    take their exact-width type, a pointer to a mirrored struct is POINTER(mirror), every other pointer (data of any
    element type, streams, opaque handles, out-pointers) is c_void_p.  It reads what lrl.h uses and nothing more: a
    declaration of another form, or a type outside these maps, raises and names the function."""
    src = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M).replace('extern "C" {', "")
    out = {}
    for m in re.finditer(r"\b(lrl_\w+)\s*\(", src):
        name = m.group(1)
        ret = re.sub(r"\s*\*\s*", "*", " ".join(re.split(r"[;{}]", src[:m.start()])[-1].split()))
        tail = re.match(r"([^()]*)\)\s*;", src[m.end():])
        if ret not in _RETURNS or tail is None:
            raise RuntimeError(f"include/lrl.h: cannot read the declaration of {name} (returns '{ret}')")
        args = []
        params = [p.strip() for p in tail.group(1).split(",")]
        for p in ([] if params == ["void"] else params):
            words = [w for w in p.replace("*", " ").split() if w != "const"]  # the type, then the name if present
            if "[" in p or not 1 <= len(words) <= 2:
                raise RuntimeError(f"include/lrl.h: cannot read parameter '{p}' of {name}")
            if p.count("*") == 1 and words[0] in MIRRORS:
                args.append(C.POINTER(MIRRORS[words[0]]))
            elif "*" in p:
                args.append(C.c_void_p)
            elif words[0] in _SCALARS:
                args.append(_SCALARS[words[0]])
            else:
                raise RuntimeError(f"include/lrl.h: parameter '{p}' of {name} has a type outside the ABI's type map")
        out[name] = (_RETURNS[ret], args)
    return out


_lib = None


def lib():
    """liblrl.so, loaded once, every function with the restype and argtypes include/lrl.h (and the headers it
    includes for the depth sensor model and the act's history shift, include/lrl_depth_sense.h and
    include/lrl_history_shift.h) declares.  Raises (no
    fallback) if it was not built, or was built from other sources than the ones in this tree (a stale binary)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"liblrl.so not built ({LIB_PATH}); run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        L.lrl_build_hash.restype = C.c_char_p
        built, want = L.lrl_build_hash().decode(), source_hash()
        # (an explicit LRL_LIB — an instrumented or A/B development build — is loaded as named)
        if built != want and not os.environ.get("LRL_LIB"):
            raise RuntimeError(f"{LIB_PATH} was built from other sources (hash {built}, tree {want}); "
                               "rebuild it: __graft_entry__.build()")
        for header in (_HEADER, _SENSE_HEADER, _SHIFT_HEADER):
            with open(header) as f:
                for name, (restype, argtypes) in signatures(f.read()).items():
                    fn = getattr(L, name)
                    fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().lrl_last_error()
        raise RuntimeError(f"liblrl error {rc}: {msg.decode() if msg else ''}")
    return rc


_dev_index_cache = {}


def stream_of(device):
    """The current HIP stream of `device` as a c_void_p (torch's raw-stream accessor: no Stream object built per call —
    a few microseconds less per launch on the host-bound upstream-reset path)."""
    idx = _dev_index_cache.get(device)
    if idx is None:
        import torch
        d = torch.device(device)
        idx = d.index if d.index is not None else torch.cuda.current_device()
        _dev_index_cache[device] = idx
    import torch
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))
