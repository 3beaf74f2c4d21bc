"""The step's numpy extras are reads of one device snapshot (lrl_sim_extras_snapshot) that is taken on demand: by the
first read of one of the eleven keys, or, if none was read, before the env next writes the state outside step (an
external reset_idx / reset, a state setter).  A step whose extras nobody reads launches nothing.

Held against the eager form (lrl.env._EAGER_EXTRAS, LRL_EXTRAS_SNAPSHOT=eager: every step launches the snapshot, as
before): the same kernel on the same state, so every key is compared bit for bit.  The launch count is the env's own
host-side counter (extras_snapshot_launches).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 64
KEYS = ("joint_pos", "joint_vel", "joint_pos_target", "body_linear_vel", "body_angular_vel", "body_linear_vel_cmd",
        "body_angular_vel_cmd", "contact_states", "foot_positions", "body_pos", "torques")


def _env(seed):
    from lrl import config as lcfg
    from lrl.env import LeggedRobotEnv
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    env = LeggedRobotEnv(DEV, cfg=cfg, num_envs=N, seed=seed)
    assert set(KEYS) == set(env._EXTRAS)
    return env


def _steps(env, seed, k=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    env.reset()
    env.commands[:, :3] = torch.rand(N, 3, generator=g, device=DEV)
    for _ in range(k):
        _, _, _, info = env.step(torch.randn(N, 12, generator=g, device=DEV) * 0.5)
    return info


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == np.float32:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    else:
        assert np.array_equal(a, b), what


def _eager(monkeypatch, seed, then=None):
    """The eleven keys of the third step on a fresh env with the eager switch (`then(env)` runs before they are read)."""
    import lrl.env as E
    monkeypatch.setattr(E, "_EAGER_EXTRAS", True)
    env = _env(seed)
    try:
        info = _steps(env, seed)
        assert env._extras_pending is None
        if then is not None:
            then(env)
        return {k: info[k] for k in KEYS}, env.extras_snapshot_launches
    finally:
        monkeypatch.setattr(E, "_EAGER_EXTRAS", False)
        env.close()


@pytest.mark.parametrize("seed", [3, 11])
def test_keys_read_lazily_equal_the_eager_snapshot(seed, monkeypatch):
    want, eager_launches = _eager(monkeypatch, seed)
    assert eager_launches == 4  # reset's step and the three steps
    env = _env(seed)
    try:
        info = _steps(env, seed)
        assert env.extras_snapshot_launches == 0, "an unread step launched a snapshot"
        got = {k: info[k] for k in KEYS}
        assert env.extras_snapshot_launches == 1, "the eleven keys share one snapshot"
        assert np.abs(got["joint_vel"]).max() > 0
        for k in KEYS:
            _same(got[k], want[k], f"seed {seed}: {k}")
    finally:
        env.close()


@pytest.mark.parametrize("how", ["reset_idx", "reset", "set_dof_state"])
def test_a_pending_snapshot_is_settled_before_an_external_write(how, monkeypatch):
    def write(env):
        if how == "reset_idx":
            env.reset_idx(torch.arange(0, N, 2, device=DEV))
        elif how == "reset":
            env.reset()
        else:
            ids = torch.arange(N, device=DEV)
            env.set_dof_state_tensor_indexed(torch.full((N, 12), 0.25, device=DEV), torch.ones(N, 12, device=DEV), ids)
    seed = 3
    # eager: the snapshot was taken by the step, so the keys hold the state before the write (reset: its own step's)
    want, _ = _eager(monkeypatch, seed, then=None if how == "reset" else write)
    env = _env(seed)
    try:
        info = _steps(env, seed)
        if how == "reset":
            # reset = reset_idx (settles the third step's snapshot: one launch) + a step, whose lazies replace them
            held = env.extras._lazy["joint_pos"]
            write(env)
            assert env.extras_snapshot_launches == 1 and env._extras_pending is not None
            got = {"joint_pos": held()}
            _same(got["joint_pos"], want["joint_pos"], "reset: the replaced entry still reads the pre-reset snapshot")
            return
        before = env.dof_pos.clone()
        assert env.extras_snapshot_launches == 0
        write(env)
        assert env.extras_snapshot_launches == 1 and env._extras_pending is None
        torch.cuda.synchronize()
        assert not torch.equal(env.dof_pos, before), "the write changed nothing: the case checks nothing"
        got = {k: info[k] for k in KEYS}
        assert env.extras_snapshot_launches == 1
        for k in KEYS:
            _same(got[k], want[k], f"{how}: {k}")
        _same(got["joint_pos"], before.cpu().numpy(), f"{how}: joint_pos is the pre-write state")
    finally:
        env.close()


def test_an_unread_step_launches_nothing_and_a_read_one_launches_once():
    env = _env(5)
    try:
        info = _steps(env, 5, k=6)
        assert env.extras_snapshot_launches == 0
        info["privileged_obs"], info["joint_vel_target"]  # not snapshot keys
        assert env.extras_snapshot_launches == 0
        a = info["torques"]
        b = info["torques"]
        info["joint_pos"]
        assert a is b and env.extras_snapshot_launches == 1
        env.step(torch.zeros(N, 12, device=DEV))
        env.reset_idx(torch.arange(4, device=DEV))  # settles the step above
        assert env.extras_snapshot_launches == 2
        env.reset_idx(torch.arange(4, device=DEV))  # nothing pending any more
        assert env.extras_snapshot_launches == 2
        env.step(torch.zeros(N, 12, device=DEV))
        for k in KEYS:  # every entry overwritten by the caller: nothing is owed
            env.extras[k] = None
        env.reset_idx(torch.arange(4, device=DEV))
        assert env.extras_snapshot_launches == 2
    finally:
        env.close()
