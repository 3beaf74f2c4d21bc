"""The navigation wrapper's native step (HighLevelControlWrapper(native=True): csrc/lrl_nav.hip) against the host-torch
wrapper, which tests/test_high_level.py pins bit-exactly to the reference's own run.

Lockstep: two envs from the same seed and low-level policy, A native and B host, fed the same scripted actions.  After
every step the low-level state must be bit-equal (a single differing command threshold or reset id shows up there), the
integer and flag buffers and the reset id list equal, and the float buffers within |a - b| <= 1e-6 S + 1e-7, S the sum
of the absolute terms of the value: each value is at most an eight-term fp32 sum of products of a <= 3-term norm,
evaluated twice in fp32 in possibly different order or contraction, 8 * 2^-24 ~ 5e-7 relative to S.  The logged means
get len(ids) * 2^-23 * mean|x| (two summation orders of len(ids) values).  Then A's float buffers are copied into B, so
the errors do not accumulate (the idiom of the physics tests)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import init_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = ("rew_buf", "dist_travelled", "lateral_vel", "backward_vel", "last_pos", "last_actions", "obs_buf", "actions")
FLAGS = ("reset_buf", "gs_buf", "time_buf", "episode_length_buf")


def _policy_net():
    from lrl.ppo.actor_critic import ActorCritic
    ac = ActorCritic(42, 18, 630, 12)
    init_params(ac)  # an untrained net with O(1) outputs: the robots stumble under +-2 m/s commands
    return ac


def _pair(n, robot, seed=3):
    from lrl.high_level import HighLevelControlWrapper
    ac = _policy_net()
    mk = lambda native: HighLevelControlWrapper.from_actor_critic(ac, num_envs=n, device=DEV, robot=robot, seed=seed,
                                                                  native=native)
    return mk(True), mk(False)


def scripted_actions(steps, n, seed):
    """[steps, n, 3] commands in [-3, 3] (so some are clamped), a third of the envs' xy scaled below the 0.2 norm, and
    no clamped xy norm within 1e-3 of 0.2 (fixed here, on the host: a pair inside the band is doubled)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3.0, 3.0, (steps, n, 3))
    small = rng.random((steps, n)) < 1.0 / 3.0
    a[..., :2] *= np.where(small, 0.03, 1.0)[..., None]
    a = a.astype(np.float32)
    norm = lambda x: np.sqrt((np.clip(x[..., :2].astype(np.float64), -2, 2) ** 2).sum(-1))
    band = np.abs(norm(a) - 0.2) < 2e-3
    a[band, :2] *= 2.0
    nn = norm(a)
    assert (np.abs(nn - 0.2) >= 1e-3).all()
    assert (nn < 0.2).any() and (nn > 0.2).any() and (np.abs(a) > 2).any()
    return a, nn


class Lockstep:
    """Steps A (native) and B (host) together and compares them after every step."""

    def __init__(self, A, B):
        self.A, self.B, self.n = A, B, A.num_envs
        self.seen = set()
        self.bars = {}  # extras key -> {name: bar} of the last reset batch of the group
        self._in_step = False
        self._ids = None
        orig_reset, orig_reward = B.reset_idx, B.compute_reward

        def reset_idx(env_ids):  # the batch's ids and what its means average, before the host path zeroes them
            if self._in_step:
                self._ids = env_ids.clone()
                ntr = B.num_train_envs
                for key, grp in (("train/episode", env_ids[env_ids < ntr]), ("eval/episode", env_ids[env_ids >= ntr])):
                    if len(grp):
                        self.bars[key] = {k: len(grp) * 2.0 ** -23 * float(v[grp].abs().mean())
                                          for k, v in B.episode_sums.items()}
            return orig_reset(env_ids)

        def compute_reward():  # S of the step's reward: the sum of its terms' magnitudes
            any_reset = bool(B.reset_buf.any())
            S = torch.zeros(self.n, device=DEV)
            for name, fn in zip(B.reward_names, B.reward_functions):
                S += (fn() * B.reward_scales[name]).abs()
            if any_reset:
                for name, fn in zip(B.terminal_reward_names, B.terminal_reward_functions):
                    S += (fn() * B.terminal_reward_scales[name]).abs()
            self._S_rew, self._any, self._ll = S, any_reset, B.ll_dones.clone()
            self._gs, self._time = B.gs_buf.clone(), B.time_buf.clone()
            return orig_reward()

        B.reset_idx, B.compute_reward = reset_idx, compute_reward
        self.check_low_level("start")

    def check_low_level(self, what):
        a, b = self.A.ll_env, self.B.ll_env
        for k in ("root_states", "dof_pos", "commands", "obs_history", "episode_length_buf", "_episode_sums"):
            x, y = getattr(a, k), getattr(b, k)
            if k == "root_states":  # (bit patterns: a -0.0 or a NaN payload counts)
                x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
            if not torch.equal(x, y):
                bad = (x != y) if x.shape[0] == self.n else (x != y).t()  # (the sum table is [rows, n])
                pytest.fail(f"{what}: low-level {k} differs in envs "
                            f"{bad.reshape(self.n, -1).any(1).nonzero().flatten().tolist()[:10]}")

    def close(self, what, a, b, S):
        bar = 1e-6 * S + 1e-7
        err = (a - b).abs()
        bad = ~(err <= bar)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside 1e-6 S + 1e-7, worst " \
                              f"{float((err - bar).max()):.3e} over the bar at {bad.nonzero()[0].tolist()}"

    def step(self, t, act):
        A, B, n = self.A, self.B, self.n
        prev = {k: v.clone() for k, v in B.episode_sums.items()}
        prev_dist = B.dist_travelled.clone()
        self._ids = None
        self._in_step = True
        oa, ra, da, xa = A.step(act)
        ob, rb, db, xb = B.step(act.clone())
        self._in_step = False
        what = f"step {t}"
        self.check_low_level(what)
        # flags, exactly; a mismatch prints the env's margins to its thresholds
        ids_a = A._ids[:int(A._cnt.item())].long()
        ids_b = self._ids if self._ids is not None else torch.zeros(0, dtype=torch.long, device=DEV)
        for k in FLAGS:
            x, y = getattr(A, k), getattr(B, k)
            if not torch.equal(x, y):
                e = int((x != y).nonzero()[0])
                bp = B._base_pos()[e]
                pytest.fail(f"{what}: {k} differs in env {e}: native {x[e].item()} host {y[e].item()}; goal margin "
                            f"{float(torch.linalg.norm(bp[:2] - B.goal_position[e]) - 0.1):.3e}, episode length "
                            f"{int(B.episode_length_buf[e])} against {B.max_episode_length}")
        assert torch.equal(da, db), what
        assert torch.equal(ids_a, ids_b), f"{what}: reset ids {ids_a.tolist()} against {ids_b.tolist()}"
        assert da.data_ptr() == A.reset_buf.data_ptr() and ra.data_ptr() == A.rew_buf.data_ptr()
        # floats
        self.close(what + " rew_buf", ra, rb, self._S_rew)
        for k, row in B.episode_sums.items():
            self.close(f"{what} episode_sums[{k}]", A.episode_sums[k], row, prev[k].abs() + (row - prev[k]).abs())
            self.close(f"{what} episode_sums_eval[{k}]", A.episode_sums_eval[k], B.episode_sums_eval[k],
                       B.episode_sums_eval[k].abs())
        self.close(what + " dist_travelled", A.dist_travelled, B.dist_travelled,
                   prev_dist.abs() + (B.dist_travelled - prev_dist).abs())
        e = B.ll_env
        pos_S = (e.root_states[:, :3].abs() + e.env_origins[:, :3].abs() + e.base_init_state[:3].abs())
        for k in ("lateral_vel", "backward_vel"):
            self.close(f"{what} {k}", getattr(A, k), getattr(B, k), getattr(B, k).abs())
        self.close(what + " last_pos", A.last_pos, B.last_pos, pos_S)
        self.close(what + " last_actions", A.last_actions, B.last_actions, B.last_actions.abs())
        self.close(what + " actions", A.actions, B.actions, B.actions.abs())
        obs_S = torch.cat([pos_S, B.obs_buf[:, 3:].abs()], 1)
        self.close(what + " obs", oa["obs"], ob["obs"], obs_S)
        assert oa["obs"].data_ptr() == A.obs_buf.data_ptr()
        assert torch.equal(oa["obs_history"], ob["obs_history"]) and torch.equal(oa["privileged_obs"], ob["privileged_obs"])
        # the logged means
        for key in ("train/episode", "eval/episode"):
            assert (key in xa) == (key in xb), f"{what}: {key} present natively {key in xa}, on the host {key in xb}"
            if key in xb:
                for k, vb in xb[key].items():
                    va, bar = xa[key][k], self.bars.get(key, {}).get(k[len("rew_"):], 0.0)
                    assert va.dim() == 0 and va.device.type == "cuda"
                    assert abs(float(va) - float(vb)) <= bar, \
                        f"{what}: {key}/{k} native {float(va)!r} host {float(vb)!r}, bar {bar:.3e}"
        # what happened, for the coverage asserts of the caller
        ntr = B.num_train_envs
        if len(ids_b) == 0:
            self.seen.add("no_reset")
        else:
            if (ids_b < ntr).any() and (ids_b >= ntr).any():
                self.seen.add("train_and_eval_together")
            if self._gs.any():
                self.seen.add("goal")
            if self._time.any():
                self.seen.add("time_out")
            if self._ll.any():
                self.seen.add("ll_fall")
            if not self._any:
                pytest.fail("ids without a set flag")
        # re-synchronise B's floats with A's
        for k in FLOATS:
            getattr(B, k).copy_(getattr(A, k))
        for k in B.episode_sums:
            B.episode_sums[k].copy_(A.episode_sums[k])
            B.episode_sums_eval[k].copy_(A.episode_sums_eval[k])


def _flip(env, ids):
    """Put the listed robots on their backs 0.3 m above their origin (the base then hits the ground: a low-level fall)."""
    r = env.ll_env.root_states
    r[ids, 2] = env.ll_env.env_origins[ids, 2] + 0.3
    r[ids, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV)
    r[ids, 7:13] = 0.0


def _close_envs(*envs):
    torch.cuda.synchronize()
    for e in envs:
        e.ll_env.env.close()


def test_lockstep_go1_every_branch():
    n, steps = 100, 60
    A, B = _pair(n, "go1")
    assert A.native and not B.native and A.num_train_envs == B.num_train_envs == 95
    acts, _ = scripted_actions(steps, n, seed=11)
    near = torch.tensor([0, 1, 2, 3, 96], device=DEV)  # four train envs and one eval env get a goal 3 cm ahead
    fall = torch.tensor([20, 21, 22, 97], device=DEV)
    A.reset(), B.reset()
    ls = Lockstep(A, B)
    for env in (A, B):
        env.max_episode_length = 7
    for t in range(steps):
        if t in (3, 40):
            for env in (A, B):
                env.goal_position[near] = env._base_pos()[near, :2] + torch.tensor([0.03, 0.0], device=DEV)
        if t in (5, 42):
            for env in (A, B):
                env.goal_position[near, 0], env.goal_position[near, 1] = 3.0, 0.0
        if t == 24:
            for env in (A, B):
                env.max_episode_length = int(10 / env.dt)
        if t in (26, 44):
            _flip(A, fall), _flip(B, fall)
        if t == 30:
            A.reset_evaluation_envs(), B.reset_evaluation_envs()
            ls.check_low_level("reset_evaluation_envs")
            for k in B.episode_sums_eval:
                assert torch.equal(A.episode_sums_eval[k], B.episode_sums_eval[k])
                assert A.episode_sums_eval[k].data_ptr() == A._sums_eval[list(B.episode_sums_eval).index(k)].data_ptr()
        ls.step(t, torch.tensor(acts[t], device=DEV))
    assert ls.seen >= {"no_reset", "train_and_eval_together", "goal", "time_out", "ll_fall"}, ls.seen
    assert "train/episode" in A.extras and "eval/episode" in A.extras
    _close_envs(A, B)


def test_lockstep_single_env():
    A, B = _pair(1, "go1")
    assert A.num_train_envs == 1
    acts, _ = scripted_actions(20, 1, seed=5)
    A.reset(), B.reset()
    ls = Lockstep(A, B)
    for env in (A, B):
        env.max_episode_length = 7
    for t in range(20):
        ls.step(t, torch.tensor(acts[t], device=DEV))
    assert ls.seen >= {"no_reset", "time_out"}, ls.seen
    assert "eval/episode" not in A.extras or "eval/episode" in B.extras
    _close_envs(A, B)


def test_lockstep_mini_cheetah_trimesh():
    """3 x 5 trimesh tiles: custom origins, the fork's root mode 0 (a reset leaves the root where it is)."""
    n, steps = 100, 16
    A, B = _pair(n, "mini_cheetah")
    assert A.ll_env.env.custom_origins and A.ll_env.env._root_mode() == 0
    acts, _ = scripted_actions(steps, n, seed=7)
    A.reset(), B.reset()
    ls = Lockstep(A, B)
    for env in (A, B):
        env.max_episode_length = 7
    for t in range(steps):
        ls.step(t, torch.tensor(acts[t], device=DEV))
    assert ls.seen >= {"no_reset", "time_out", "train_and_eval_together"}, ls.seen
    _close_envs(A, B)


def test_lockstep_other_reward_scales(monkeypatch):
    """terminal_distance_covered = 0.5 shows the "some env ends" condition in every env's reward; a zero step scale
    drops its term (and its sum row)."""
    from lrl import high_level
    monkeypatch.setattr(high_level.reward_scales, "terminal_distance_covered", 0.5)
    monkeypatch.setattr(high_level.reward_scales, "lateral_vel", 0.0)
    n, steps = 100, 20
    A, B = _pair(n, "go1")
    assert "lateral_vel" not in A.episode_sums and "terminal_distance_covered" in A.episode_sums
    assert list(A.episode_sums) == list(B.episode_sums) and A._sums.shape == (len(B.episode_sums), n)
    acts, _ = scripted_actions(steps, n, seed=13)
    A.reset(), B.reset()
    ls = Lockstep(A, B)
    for env in (A, B):
        env.max_episode_length = 7
    near = torch.tensor([4, 5], device=DEV)
    for t in range(steps):
        if t == 2:
            for env in (A, B):
                env.goal_position[near] = env._base_pos()[near, :2] + torch.tensor([0.03, 0.0], device=DEV)
        if t == 4:
            for env in (A, B):
                env.goal_position[near, 0], env.goal_position[near, 1] = 3.0, 0.0
        ls.step(t, torch.tensor(acts[t], device=DEV))
    assert ls.seen >= {"no_reset", "goal", "time_out"}, ls.seen
    _close_envs(A, B)


def _buffers(env):
    out = {k: getattr(env, k).clone() for k in FLOATS + FLAGS + ("goal_position",)}
    out["sums"], out["sums_eval"] = env._sums.clone(), env._sums_eval.clone()
    out["ids"], out["cnt"] = env._ids.clone(), env._cnt.clone()
    for key in ("train/episode", "eval/episode"):
        if key in env.extras:
            out[key] = torch.stack(list(env.extras[key].values()))
    return out


def test_native_runs_are_bit_identical_and_in_place():
    from lrl.high_level import HighLevelControlWrapper
    n, steps = 100, 20
    acts, _ = scripted_actions(steps, n, seed=17)
    runs = []
    for _ in range(2):
        env = HighLevelControlWrapper.from_actor_critic(_policy_net(), num_envs=n, device=DEV, robot="go1", seed=3,
                                                        native=True)
        env.reset()
        env.max_episode_length = 7
        ptr = env.get_observations()["obs"].data_ptr()
        for t in range(steps):
            if t == 10:  # a caller's rebinding (Runner.learn(init_at_random_ep_len=True)) is honoured on the next step
                env.episode_length_buf = bound = torch.full_like(env.episode_length_buf, 5)
            obs, rew, done, extras = env.step(torch.tensor(acts[t], device=DEV))
            assert obs["obs"].data_ptr() == ptr == env.get_observations()["obs"].data_ptr()
            if t == 10:  # counted in the new tensor (6), or reset in it (an env that fell in this step)
                assert env.episode_length_buf is bound and (bound == 6).any() and ((bound == 6) | (bound == 0)).all()
            if t == 12:  # 8 > 7: the envs counted from 5 time out and are reset in the rebound tensor
                assert env.time_buf.any() and (bound[env.time_buf] == 0).all()
        runs.append(_buffers(env))
        _close_envs(env)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        x, y = runs[0][k], runs[1][k]
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), k


def test_refusals():
    from lrl import _abi
    from lrl import config as lcfg
    from lrl.env import LeggedRobotEnv
    from lrl.high_level import HighLevelControlWrapper
    from lrl.history import HistoryWrapper
    cfg = lcfg.make_cfg()
    lcfg.config_go1(cfg)
    cfg.env.num_envs = 2
    up = HistoryWrapper(LeggedRobotEnv(DEV, cfg=cfg, legacy_fork=False))
    with pytest.raises(ValueError, match="legacy_fork"):
        HighLevelControlWrapper(up, lambda ob: torch.zeros(2, 12, device=DEV), native=True)
    up.env.close()
    env = HighLevelControlWrapper.from_actor_critic(_policy_net(), num_envs=2, device=DEV, native=True)
    with pytest.raises(ValueError, match="num_envs"):
        HighLevelControlWrapper(env.ll_env, env.low_level_policy, num_envs=1, native=True)
    L, sim = _abi.lib(), env.ll_env.env._sim
    scratch = torch.zeros(64, device=DEV)
    act = torch.zeros(2, 3, device=DEV)

    def state():
        v = env._nav_bind()
        v.means_train = v.means_eval = v.means_ll = scratch.data_ptr()
        return v
    calls = (lambda v: L.lrl_nav_begin_step(sim, C.byref(v), C.c_void_p(act.data_ptr()), None),
             lambda v: L.lrl_nav_end_step(sim, C.byref(v), 0, 1, 0.0, 0.0, 0.0, 0.0, None))
    before = {k: getattr(env, k).clone() for k in FLOATS + FLAGS}
    for call in calls:
        v = state()
        v.n += 1
        assert call(v) == -1 and b"lrl_nav_state.n 3" in L.lrl_last_error()
        v = state()
        v.obs_buf = None
        assert call(v) == -1 and b"obs_buf is null" in L.lrl_last_error()
        for field, value, msg in (("num_train_envs", 0, b"num_train_envs"), ("num_train_envs", 3, b"num_train_envs"),
                                  ("num_terminal_terms", 24, b"at most 24")):
            v = state()
            setattr(v, field, value)
            assert call(v) == -1 and msg in L.lrl_last_error()
        v = state()
        v.term[0] = len(_abi.NAV_TERMS)
        assert call(v) == -1 and b"no lrl_nav_term" in L.lrl_last_error()
    torch.cuda.synchronize()
    for k, want in before.items():  # a refused call launched nothing
        assert torch.equal(getattr(env, k), want), k
    _close_envs(env)


def test_runner_learns_over_the_native_wrapper(tmp_path):
    from lrl.high_level import HighLevelControlWrapper
    from lrl.hlp import Runner, RunnerArgs
    from lrl.ppo.actor_critic import ActorCritic as LowLevelActorCritic
    from lrl.ppo.runner import Logger
    env = HighLevelControlWrapper.from_actor_critic(LowLevelActorCritic(42, 18, 630, 12), num_envs=64, device=DEV,
                                                    robot="go1", seed=3, native=True)
    steps = RunnerArgs.num_steps_per_env
    RunnerArgs.num_steps_per_env = 8
    try:
        runner = Runner(env, device=DEV, logger=Logger(str(tmp_path)))
    finally:
        RunnerArgs.num_steps_per_env = steps
    assert runner.alg.fused and runner.alg.storage.num_envs == env.num_train_envs == 60
    env.max_episode_length = 5  # every env times out inside the 8 steps: a reset batch on the device
    runner.learn(1, init_at_random_ep_len=True, eval_freq=1, eval_expert=True)
    torch.cuda.synchronize()
    st = runner.alg.storage
    assert torch.isfinite(st.rewards).all() and st.dones.dtype in (torch.uint8, torch.bool)
    assert int(env._cnt.item()) >= 0 and (env.episode_length_buf <= 8).all()
    summary = runner.logger.summaries[-1]
    assert np.isfinite(summary["train/episode/rew_total/mean"])
    assert isinstance(env.extras["train/episode"]["rew_total"], torch.Tensor)
    assert env.extras["train/episode"]["rew_total"].device.type == "cuda"
    _close_envs(env)
