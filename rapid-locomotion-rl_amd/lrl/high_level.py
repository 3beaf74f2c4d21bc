"""HighLevelControlWrapper — the reference's second client of the env API (scripts/high_level_play.py:30-363).

A high-level policy outputs body-velocity commands (3 actions) every policy step; a frozen low-level locomotion
policy turns the env's observations into joint targets; the wrapper keeps its own observation (base position
relative to the start, base velocities, last command, goal), rewards (distance to the goal, action rate,
lateral / backward velocity; terminal rewards for reaching the goal, low-level falls and time-outs), episode
bookkeeping and resets.  By default all of it is host-side torch on the env's device, as in the reference; the env
step and the low-level policy run on the native path (``LeggedRobotEnv.step`` = one fused HIP launch, the low-level
policy through ``ActorCritic.act_student_fused`` = the adaptation module + actor GEMM chain).

``native=True`` runs the wrapper's own step on the device as well (csrc/lrl_nav.hip: ``lrl_nav_begin_step`` before the
low-level policy, ``lrl_nav_end_step`` after ``ll_env.step``): six launches and no host read per step in place of about
a hundred torch ops and several host waits.  The wrapper's buffers stay torch tensors, rewritten in place; the host
methods that run rarely (``reset``, ``reset_idx``, ``reset_evaluation_envs``) work on the same buffers.  The host path
is the check for the native one (tests/test_nav_native_gpu.py).

The reference's constructor loads the newest ml_logger run (``_load_env``, :251-334); here the low-level env and
policy are passed in, or built by ``from_actor_critic`` with the evaluation overrides of ``_load_env`` (domain
randomisation off, 3 x 5 terrain tiles, no border).
"""
import ctypes as C

import torch

from ._abi import NAV_TERMS


class reward_scales:  # high_level_play.py:16-28
    # terminal rewards
    terminal_distance_covered = 0.00
    terminal_distance_gs = 5.0
    terminal_ll_reset = -2.0
    terminal_time_out = -1.0
    # step rewards
    distance = -0.1
    action_rate = -0.01
    lateral_vel = -0.05
    backward_vel = -0.005


_NAV_TERM_IDS = {k: i for i, k in enumerate(NAV_TERMS)}  # reward name -> enum lrl_nav_term


class HighLevelControlWrapper:
    def __init__(self, ll_env, low_level_policy, num_envs=None, device=None, goal=(3.0, 0.0), native=False):
        """ll_env: a HistoryWrapper over LeggedRobotEnv; low_level_policy: obs dict -> joint actions.
        native: run ``step`` on the device (refused, never replaced by the host path, where it cannot)."""
        self.native = bool(native)
        if getattr(getattr(getattr(ll_env, "env", ll_env), "cfg", None), "depth", None) is not None:
            # Both paths go through LeggedRobotEnv.step, whose depth refresh follows the step's own resets; this wrapper
            # resets the low-level envs after that step (reset_idx / lrl_nav_end_step), so a reset env would keep its
            # previous episode's image until its next redraw.  Refused rather than served stale.
            raise ValueError("HighLevelControlWrapper: the low-level env's cfg has the depth camera group Cfg.depth; "
                             "the wrapper resets envs after the low-level step's depth refresh, so the images of reset "
                             "envs would be stale (not supported yet)")
        if self.native:
            self._native_check(ll_env, num_envs)
        self.ll_env = ll_env
        self.low_level_policy = low_level_policy
        self.device = device or ll_env.device
        self.num_obs = 14
        self.num_actions = 3
        self.max_episode_length_s = 10
        self.num_privileged_obs = 18
        self.num_obs_history = 16
        self.num_envs = num_envs or ll_env.num_envs
        self.num_train_envs = max(1, int(self.num_envs * 0.95))
        self.dt = ll_env.dt
        self.max_episode_length = int(self.max_episode_length_s / ll_env.dt)
        self.ll_env.commands[:, :3] = 0.0
        self.ll_obs = self.ll_env.reset()
        self.ll_rew = self.ll_env.rew_buf
        n, d = self.num_envs, self.device
        z = lambda *s, dtype=torch.float: torch.zeros(*s, device=d, dtype=dtype)
        self.obs_buf = z(n, self.num_obs)
        self.rew_buf = z(n)
        self.discount_rew_buf = z(n) + 1.0
        self.gs_buf = z(n, dtype=torch.bool)
        self.reset_buf = z(n, dtype=torch.bool)
        self.time_buf = z(n, dtype=torch.bool)
        self.episode_length_buf = z(n, dtype=torch.int)
        self.actions = z(n, self.num_actions)
        self.last_actions = z(n, self.num_actions)
        self.last_pos = self._base_pos()
        self.dist_travelled = z(n)
        self.lateral_vel = z(n)
        self.backward_vel = z(n)
        self.privileged_obs_buf = z(n, self.num_privileged_obs)
        self.obs_history = z(n, self.num_obs_history)
        self.goal_position = z(n, 2)
        self.goal_position[:, 0] = goal[0]
        self.goal_position[:, 1] = goal[1]
        self.extras = {}
        if self.native:
            from .env import _LazyExtras
            self.extras = _LazyExtras(self)
        attrs = {k: v for k, v in vars(reward_scales).items() if not k.startswith("__")}
        self.reward_scales = {k: v for k, v in attrs.items() if not k.startswith("terminal")}
        self.terminal_reward_scales = {k: v for k, v in attrs.items() if k.startswith("terminal")}
        self._prepare_reward_function()
        if self.native:
            self._native_init()

    @classmethod
    def from_actor_critic(cls, actor_critic, num_envs=1, device="cuda:0", robot="go1", seed=0, native=False):
        """The environment of _load_env (high_level_play.py:251-334): config_go1 with every domain randomisation
        off, 3 x 5 terrain tiles without border; the low-level policy is ``actor_critic``'s student path."""
        from . import config as lcfg
        from .env import LeggedRobotEnv
        from .history import HistoryWrapper
        cfg = lcfg.make_cfg()
        (lcfg.config_go1 if robot == "go1" else lcfg.config_mini_cheetah)(cfg)
        dr = cfg.domain_rand
        for k in ("push_robots", "randomize_friction", "randomize_restitution", "randomize_motor_strength",
                  "randomize_base_mass", "randomize_Kd_factor", "randomize_Kp_factor", "randomize_com_displacement"):
            setattr(dr, k, False)
        cfg.env.num_envs = num_envs
        cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 3, 5, 0
        cfg.terrain.max_init_terrain_level = min(cfg.terrain.max_init_terrain_level, cfg.terrain.num_rows - 1)
        env = HistoryWrapper(LeggedRobotEnv(device, cfg=cfg, seed=seed))
        actor_critic = actor_critic.to(env.device)

        def policy(ob):  # ActorCritic.act_inference (actor_critic.py:96-99) on the native student path
            return actor_critic.act_student_fused(ob["obs"].contiguous(), ob["obs_history"])[0]

        return cls(env, policy, num_envs=num_envs, device=env.device, native=native)

    def _base_pos(self):
        e = self.ll_env
        return e.root_states[:, :3] - e.env_origins[:, :3] - e.base_init_state[:3]

    def _prepare_reward_function(self):
        """high_level_play.py:88-129: zero scales dropped, step rewards x dt, terminal rewards as they are."""
        for key in list(self.reward_scales):
            if self.reward_scales[key] == 0:
                self.reward_scales.pop(key)
            else:
                self.reward_scales[key] *= self.dt
        for key in list(self.terminal_reward_scales):
            if self.terminal_reward_scales[key] == 0:
                self.terminal_reward_scales.pop(key)
        self.reward_names = list(self.reward_scales)
        self.reward_functions = [getattr(self, "_reward_" + k) for k in self.reward_names]
        self.terminal_reward_names = list(self.terminal_reward_scales)
        self.terminal_reward_functions = [getattr(self, "_reward_" + k) for k in self.terminal_reward_names]
        names = [*self.reward_scales, *self.terminal_reward_scales]
        n, d = self.num_envs, self.device
        if self.native:  # one [terms + 1, n] table each, "total" last; the dicts are its rows
            bad = [k for k in names if k not in _NAV_TERM_IDS]
            if bad:
                raise ValueError(f"native=True: no device term for the reward(s) {bad}")
            self._sums = torch.zeros(len(names) + 1, n, device=d)
            self._sums_eval = -torch.ones(len(names) + 1, n, device=d)
            self._sums_eval[-1] = 0.0
            self.episode_sums = dict(zip(names + ["total"], self._sums.unbind(0)))
            self.episode_sums_eval = dict(zip(names + ["total"], self._sums_eval.unbind(0)))
            return
        self.episode_sums = {k: torch.zeros(n, device=d) for k in names}
        self.episode_sums["total"] = torch.zeros(n, device=d)
        self.episode_sums_eval = {k: -torch.ones(n, device=d) for k in names}
        self.episode_sums_eval["total"] = torch.zeros(n, device=d)

    def step(self, actions):
        """high_level_play.py:131-150: the command is clipped to [-2, 2] and its xy part zeroed below 0.2; the
        low-level policy acts on the previous low-level observation, then the env steps with the new command."""
        if self.native:
            return self._step_native(actions)
        self.actions = torch.clamp(actions, -2, 2)
        self.actions[:, :2] *= (torch.norm(self.actions[:, :2], dim=1) > 0.2).unsqueeze(1)
        with torch.no_grad():
            ll_actions = self.low_level_policy(self.ll_obs)
        self.ll_env.commands[:, :3] = self.actions
        self.ll_obs, self.ll_rew, self.ll_dones, self.ll_info = self.ll_env.step(ll_actions)
        self.episode_length_buf += 1
        self.post_physics_step()
        env_ids = self.check_termination()
        self.compute_reward()
        self.reset_idx(env_ids)
        self.compute_observations()
        self.last_actions[:] = self.actions[:]
        return self.get_observations(), self.rew_buf, self.reset_buf, self.extras

    def post_physics_step(self):
        self.lateral_vel[:] = 0.0
        self.backward_vel[:] = 0.0
        self.base_pos = self._base_pos()
        self.dist_travelled[:] += torch.abs(torch.linalg.norm(self.base_pos - self.last_pos, dim=-1))
        self.lateral_vel[:] = self.ll_env.base_lin_vel[:, 1]
        self.backward_vel[:] = torch.clamp_max(self.ll_env.base_lin_vel[:, 0], 0)

    def compute_observations(self):
        self.base_pos = self._base_pos()
        self.base_lin_vel = self.ll_env.base_lin_vel
        self.base_ang_vel = self.ll_env.base_ang_vel
        parts = [self.base_pos, self.base_lin_vel, self.base_ang_vel, self.actions, self.goal_position]
        if self.native:  # (get_observations hands out the same tensor every step)
            torch.cat(parts, dim=-1, out=self.obs_buf)
        else:
            self.obs_buf = torch.cat(parts, dim=-1)
        self.last_pos[:] = self.base_pos[:]

    def compute_reward(self):
        self.rew_buf[:] = 0.0
        for name, fn in zip(self.reward_names, self.reward_functions):
            rew = fn() * self.reward_scales[name]
            self.rew_buf += rew
            self.episode_sums[name] += rew
        if len(self.reset_buf.nonzero(as_tuple=False)) > 0:  # terminal rewards in steps where some env ends
            for name, fn in zip(self.terminal_reward_names, self.terminal_reward_functions):
                rew = fn() * self.terminal_reward_scales[name]
                self.rew_buf += rew
                self.episode_sums[name] += rew
        self.episode_sums["total"] += self.rew_buf

    def check_termination(self):
        self.gs_buf = torch.linalg.norm(self.base_pos[:, :2] - self.goal_position, dim=-1) < 0.1
        self.time_buf = self.episode_length_buf > self.max_episode_length
        self.reset_buf |= self.ll_dones
        self.reset_buf |= self.gs_buf
        self.reset_buf |= self.time_buf
        return self.reset_buf.nonzero(as_tuple=False).flatten()

    def reset_idx(self, env_ids):
        if len(env_ids) == 0:
            return self.obs_buf
        tr = env_ids[env_ids < self.num_train_envs]
        if len(tr) > 0:
            self.extras["train/episode"] = {}
            for key in self.episode_sums:
                self.extras["train/episode"]["rew_" + key] = torch.mean(self.episode_sums[key][tr])
                self.episode_sums[key][tr] = 0
        ev = env_ids[env_ids >= self.num_train_envs]
        if len(ev) > 0:
            self.extras["eval/episode"] = {}
            for key in self.episode_sums_eval:
                unset = ev[self.episode_sums_eval[key][ev] == -1]
                self.episode_sums_eval[key][unset] = self.episode_sums[key][unset]
                self.extras["eval/episode"]["rew_" + key] = torch.mean(self.episode_sums[key][ev])
                self.episode_sums[key][ev] = 0
        self.ll_env.reset_idx(env_ids)
        self.rew_buf[env_ids] = 0.0
        self.episode_length_buf[env_ids] = 0
        self.lateral_vel[env_ids] = 0.0
        self.backward_vel[env_ids] = 0.0
        self.dist_travelled[env_ids] = 0.0
        e = self.ll_env
        self.last_pos[env_ids] = e.root_states[env_ids, :3] - e.env_origins[env_ids, :3] - e.base_init_state[:3]
        self.compute_observations()
        self.reset_buf[env_ids] = False
        return self.get_observations()

    def reset(self):
        self.reset_idx(torch.arange(0, self.num_envs, 1, dtype=torch.long, device=self.device))
        return self.get_observations()

    def reset_evaluation_envs(self):
        ids = torch.arange(self.num_train_envs, self.num_envs, 1, dtype=torch.long, device=self.device)
        self.extras.setdefault("eval/episode", {})
        for key in self.episode_sums_eval:
            unset = ids[self.episode_sums_eval[key][ids] == -1]
            self.episode_sums_eval[key][unset] = self.episode_sums[key][unset]
            s = self.episode_sums_eval[key]
            self.extras["eval/episode"]["rew_" + key] = torch.mean(s[s != -1])
        self.reset_idx(ids)
        if self.native:  # (the dict's tensors are rows of the table the kernels read)
            self._sums_eval.fill_(-1.0)
            return self.get_observations()
        for key in self.episode_sums_eval:
            self.episode_sums_eval[key] = -torch.ones(self.num_envs, device=self.device)
        return self.get_observations()

    def get_observations(self):
        return {"obs": self.obs_buf, "privileged_obs": self.privileged_obs_buf, "obs_history": self.obs_history}

    # ---- the step on the device (csrc/lrl_nav.hip) ----
    @staticmethod
    def _native_check(ll_env, num_envs):
        """What ``native=True`` needs of the low-level env; each miss is an error naming it."""
        from .env import LeggedRobotEnv
        from .history import HistoryWrapper
        e = getattr(ll_env, "env", None)
        if not isinstance(ll_env, HistoryWrapper) or not isinstance(e, LeggedRobotEnv) or not getattr(e, "_sim", None):
            raise TypeError("native=True needs a HistoryWrapper over a LeggedRobotEnv with a sim as ll_env, got "
                            f"{type(ll_env).__name__}")
        if e.eval_cfg is not None:
            raise ValueError("native=True: the low-level env has an eval group (eval_cfg), which resets per group on "
                             "the host")
        import torch.distributed as dist
        if e._dist is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise ValueError("native=True: several ranks share collective curriculum steps on the host")
        if not e.legacy_fork:
            raise ValueError("native=True needs legacy_fork=True: with legacy_fork=False the low-level step resets and "
                             "resamples on its own")
        if e.custom_origins and e.cfg.terrain.curriculum:
            raise ValueError("native=True: the terrain curriculum moves env origins at every reset on the host")
        if num_envs is not None and num_envs != ll_env.num_envs:
            raise ValueError(f"native=True: num_envs {num_envs} differs from the low-level env's {ll_env.num_envs}")

    def _native_init(self):
        from . import _abi
        e = self.ll_env.env
        self._abi, self._L, self._e = _abi, _abi.lib(), e
        n, d = self.num_envs, self.device
        self.last_pos = self.last_pos.contiguous()  # (_base_pos() keeps the sim's [field][env] strides)
        self._ids = torch.zeros(n, dtype=torch.int32, device=d)   # the last step's reset ids, ascending
        self._cnt = torch.zeros(1, dtype=torch.int32, device=d)   # and their count
        self._blk = torch.zeros((n + _abi.NAV_BLOCK - 1) // _abi.NAV_BLOCK, dtype=torch.int32, device=d)
        self._nav = _abi.LrlNavState()
        nan = lambda k: torch.full((k,), float("nan"), device=d)
        R = self._sums.shape[0]
        self._prev = {"train/episode": nan(R), "eval/episode": nan(R), "ll": nan(e._episode_sums.shape[0])}
        self._seen = {"train/episode": False, "eval/episode": False}
        self._pub = {}  # key -> the dict this path published last

    def _nav_bind(self):
        """Pointers and scalars of the state, read from the attributes at every step (callers rebind them)."""
        v = self._nav
        for k in ("obs_buf", "rew_buf", "reset_buf", "gs_buf", "time_buf", "episode_length_buf", "actions",
                  "last_actions", "last_pos", "dist_travelled", "lateral_vel", "backward_vel", "goal_position"):
            t = getattr(self, k)
            if not t.is_contiguous():
                raise ValueError(f"native step: {k} must be contiguous")
            setattr(v, k, t.data_ptr())
        if self.episode_length_buf.dtype != torch.int32:
            raise TypeError(f"native step: episode_length_buf must be int32, got {self.episode_length_buf.dtype}")
        v.episode_sums, v.episode_sums_eval = self._sums.data_ptr(), self._sums_eval.data_ptr()
        v.ids, v.count, v.block_counts = self._ids.data_ptr(), self._cnt.data_ptr(), self._blk.data_ptr()
        v.n, v.num_train_envs, v.max_episode_length = self.num_envs, self.num_train_envs, int(self.max_episode_length)
        v.num_step_terms, v.num_terminal_terms = len(self.reward_names), len(self.terminal_reward_names)
        for i, k in enumerate(self.reward_names):
            v.term[i], v.scale[i] = _NAV_TERM_IDS[k], self.reward_scales[k]
        for i, k in enumerate(self.terminal_reward_names, len(self.reward_names)):
            v.term[i], v.scale[i] = _NAV_TERM_IDS[k], self.terminal_reward_scales[k]
        v.base_init_state[:] = self._e._P.base_init_state[:3]
        v.command_threshold, v.goal_threshold = 0.2, 0.1
        return v

    def _step_native(self, actions):
        """step() with the wrapper's own work in six launches: begin_step, [low-level policy, ll_env.step,] end_step."""
        from .env import _logged_prev
        _abi, L, e = self._abi, self._L, self._e
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            actions = actions.to(self.device, torch.float32).contiguous()
        if actions.shape != (self.num_envs, self.num_actions):
            raise ValueError(f"actions must be [{self.num_envs}, {self.num_actions}], got {tuple(actions.shape)}")
        v = self._nav_bind()
        # This step's logged means land in a fresh buffer (a group without a reset batch receives the previous step's),
        # so a published dict holds values no later step overwrites, as the reference's fresh tensors per reset batch.
        R, Rl = self._sums.shape[0], e._episode_sums.shape[0]
        pub = torch.empty(2 * R + Rl, device=self.device)
        slots = {"train/episode": pub[:R], "eval/episode": pub[R:2 * R], "ll": pub[2 * R:]}
        prev, names = self._prev, self.episode_sums
        for key in self._seen:  # continue from what the host methods logged last (reset, reset_evaluation_envs)
            prev[key], out = _logged_prev(self.extras, key, names, prev[key], self._pub.get(key))
            self._seen[key] = self._seen[key] or out
        prev["ll"], _ = _logged_prev(e.extras, "train/episode", e.episode_sums, prev["ll"], e._nav_log["ep"])
        order = ("train/episode", "eval/episode", "ll")
        v.means_train, v.means_eval, v.means_ll = (slots[k].data_ptr() for k in order)
        v.prev_train, v.prev_eval, v.prev_ll = (prev[k].data_ptr() for k in order)
        _abi.check(L.lrl_nav_begin_step(e._sim, C.byref(v), actions.data_ptr(), e._stream()))
        with torch.no_grad():
            ll_actions = self.low_level_policy(self.ll_obs)
        self.ll_obs, self.ll_rew, self.ll_dones, self.ll_info = self.ll_env.step(ll_actions)
        e._settle_extras()  # lrl_nav_end_step resets envs: the low-level step's extras hold the state before that
        t = e.cfg.terrain
        reset_args = (e._root_mode(), float(t.x_init_range), float(t.y_init_range) - float(t.x_init_range),
                      float(t.x_init_offset), float(t.y_init_offset), e._stream())
        c = e.cfg.commands
        if (c.command_curriculum or c.yaw_command_curriculum) and \
                e.common_step_counter % e.cfg.env.max_episode_length == 0:
            # the uniform command-range curriculum's step (once per episode length): it reads the batch's tracking sums
            # on the host before they are zeroed, so the ids are made first and their count read (a stream sync)
            _abi.check(L.lrl_nav_end_step(e._sim, C.byref(v), _abi.NAV_ONLY_FLAGS, *reset_args))
            k = int(self._cnt.item())
            if k:
                e.update_command_curriculum(self._ids[:k].long(), e.cfg)
            _abi.check(L.lrl_nav_end_step(e._sim, C.byref(v), _abi.NAV_ONLY_RESET, *reset_args))
        else:
            _abi.check(L.lrl_nav_end_step(e._sim, C.byref(v), 0, *reset_args))
        self._prev = slots
        keys = ["train/episode"] + (["eval/episode"] if self.num_envs > self.num_train_envs else [])
        for key in keys:
            means = slots[key]
            ep = self._pub[key] = {"rew_" + k: m for k, m in zip(self.episode_sums, means.unbind(0))}
            if self._seen[key]:
                self.extras[key] = ep
            else:  # the key appears with the group's first reset batch (the means are NaN until then); deciding
                # that reads one device value, on access only
                def seen(key=key, m0=means[0]):
                    if bool(torch.isnan(m0).item()):
                        return False
                    self._seen[key] = True
                    return True
                self.extras.set_conditional(key, ep, seen)
        e._publish_reset_batch_dev(slots["ll"])
        return self.get_observations(), self.rew_buf, self.reset_buf, self.extras

    # ---- rewards (high_level_play.py:339-363) ----
    def _reward_distance(self):
        return torch.linalg.norm(self.last_pos[:, :2] - self.goal_position, dim=-1)

    def _reward_lateral_vel(self):
        return torch.square(self.lateral_vel)

    def _reward_backward_vel(self):
        return torch.square(self.backward_vel)

    def _reward_action_rate(self):
        return torch.sum(torch.square(self.last_actions - self.actions), dim=1)

    def _reward_terminal_ll_reset(self):
        return self.ll_dones * 1.0

    def _reward_terminal_distance_gs(self):
        return self.gs_buf * 1.0

    def _reward_terminal_distance_covered(self):
        return self.dist_travelled

    def _reward_terminal_time_out(self):
        return self.time_buf * 1.0
