"""GPU side of the observation-layout switches (env.observe_only_ang_vel / observe_only_lin_vel / observe_yaw,
commands.global_reference):

* the step kernel against the REFERENCE (tests/golden/post_physics_obs_*.npz, make_golden_obs.py), replayed as
  test_env_gpu.py::test_post_physics_matches_reference replays its fixtures, at the same bars;
* the terrain-mesh build's row writers and the upstream-reset path (observe_kernel) against a numpy float32
  restatement of the row from the env's own post-step tensors (obs_layouts.expected_rows);
* the act / update GEMM chains at the new widths 45, 49 and 55, and one Runner.learn iteration at 55.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import autograd_minibatch, golden, init_params
from lrl import _abi
from lrl import config as lcfg
from obs_layouts import ALL_ON, CASES, expected_rows, heading64

pytestmark = pytest.mark.gpu


def _cfg(robot, n, **over):
    cfg = lcfg.make_cfg()
    (lcfg.config_mini_cheetah if robot == "mc" else lcfg.config_go1)(cfg)
    cfg.env.num_envs = n
    for k, v in over.items():
        node = cfg
        *ps, leaf = k.split(".")
        for p in ps:
            node = getattr(node, p)
        setattr(node, leaf, v)
    return cfg


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_post_physics_matches_reference(case):
    """3 steps of the reference's LeggedRobot.step per case.  yaw_global / all: the world-frame velocity block, the
    yaw entry over unclipped, clipped-high and clipped-low headings, and the world-frame tracking_lin_vel reward (rew,
    episode and command sums)."""
    from lrl.env import LeggedRobotEnv
    robot, fixture, over = CASES[case]
    g = golden(fixture)
    n = g["root_in"].shape[1]
    env = LeggedRobotEnv("cuda:0", cfg=_cfg(robot, n, **over))
    assert env.reward_names == [str(k) for k in g["reward_names"]]
    assert env.num_obs == g["obs"].shape[2]
    env.friction_coeffs[:] = _dev(g["init_friction"])
    env.restitutions[:] = _dev(g["init_restitution"])
    env.payloads[:] = _dev(g["init_payload"])
    env.com_displacements[:] = _dev(g["init_com"])
    env.motor_strengths[:] = _dev(g["init_motor_strengths"])
    env.Kp_factors[:] = 1.0
    env.Kd_factors[:] = 1.0
    env.episode_length_buf[:] = _dev(g["init_episode_length"], torch.int32)
    env._episode_sums[:] = _dev(g["init_episode_sums"])
    env._command_sums[:] = _dev(g["init_command_sums"])
    env.feet_air_time[:] = _dev(g["init_feet_air_time"])
    env._last_contacts_u8[:] = _dev(g["init_last_contacts"], torch.uint8)
    env.last_actions[:] = _dev(g["init_last_actions"])
    env.last_dof_vel[:] = _dev(g["init_last_dof_vel"])
    L = _abi.lib()
    for s in range(g["root_in"].shape[0]):
        env.root_states[:] = _dev(g["root_in"][s])
        env.dof_pos[:] = _dev(g["dof_pos_in"][s])
        env.dof_vel[:] = _dev(g["dof_vel_in"][s])
        env.contact_forces[:] = _dev(g["contact_in"][s])
        env.commands[:] = _dev(g["commands"][s])
        act = _dev(g["actions"][s])
        noise = _dev(g["noise_u"][s])
        dr = _dev(np.nan_to_num(g["ms_u"][s]))
        push = _dev(np.nan_to_num(g["push_u"][s]))
        _abi.check(L.lrl_sim_inject_push_uniforms(env._sim, C.c_void_p(push.data_ptr())))
        _abi.check(L.lrl_sim_inject_uniforms(env._sim, C.c_void_p(noise.data_ptr()), C.c_void_p(dr.data_ptr())))
        _abi.check(L.lrl_sim_step(env._sim, C.c_void_p(act.data_ptr()), C.c_uint32(_abi.STEP_INJECT_UNIFORM),
                                  env._stream()))
        torch.cuda.synchronize()
        obs = _np(env.obs_buf)
        if "env.observe_yaw" in over:  # (measured before asserted)
            col = obs.shape[1] - 1
            print(f"{case} step {s}: yaw column max |kernel - reference| "
                  f"{np.abs(obs[:, col] - g['obs'][s][:, col]).max():.3e}")
        np.testing.assert_array_equal(_np(env.torques), g["torques"][s])
        np.testing.assert_array_equal(_np(env.joint_pos_target), g["joint_pos_target"][s])
        np.testing.assert_array_equal(_np(env.root_states), g["root_out"][s])
        np.testing.assert_array_equal(_np(env.motor_strengths), g["motor_strengths"][s])
        np.testing.assert_array_equal(_np(env._reset_u8), g["reset"][s])
        np.testing.assert_array_equal(_np(env.episode_length_buf), g["episode_length"][s])
        np.testing.assert_array_equal(_np(env.last_contacts), g["last_contacts"][s])
        tol = dict(rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(_np(env.base_lin_vel), g["base_lin_vel"][s], **tol)
        np.testing.assert_allclose(_np(env.base_ang_vel), g["base_ang_vel"][s], **tol)
        np.testing.assert_allclose(_np(env.projected_gravity), g["projected_gravity"][s], **tol)
        np.testing.assert_allclose(_np(env.feet_air_time), g["feet_air_time"][s], **tol)
        np.testing.assert_allclose(_np(env.rew_buf), g["rew"][s], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(_np(env._episode_sums), g["episode_sums"][s], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(_np(env._command_sums), g["command_sums"][s], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(obs, g["obs"][s], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(_np(env.privileged_obs_buf), g["priv"][s], rtol=1e-6, atol=1e-6)
    env.close()


def _spin(env, rng):
    """Give every env a uniform yaw in (-pi, pi) (upright, the rest of its state as it is): the spawn heading is 0."""
    yaw = rng.uniform(-np.pi, np.pi, env.num_envs)
    q = np.zeros((env.num_envs, 4), np.float32)
    q[:, 2], q[:, 3] = np.sin(yaw / 2), np.cos(yaw / 2)
    env.root_states[:, 3:7] = _dev(q)


def _assert_rows(env, cfg, rows=None, what=""):
    """obs_buf rows == the restatement from the env's post-step tensors; no heading within 1e-3 of the wrap."""
    h = heading64(_np(env.root_states)[:, 3:7])
    assert np.all(np.pi - np.abs(h) > 1e-3), "a heading sits on the +-pi wrap at this seed"
    got, ref = _np(env.obs_buf), expected_rows(env, cfg)
    assert got.shape == ref.shape
    sel = slice(None) if rows is None else rows
    np.testing.assert_allclose(got[sel], ref[sel], rtol=1e-6, atol=1e-6, err_msg=what)
    return h


def test_terrain_mesh_rows_match_restatement():
    """The terrain-mesh build (one quad per env writes the whole row): 64 Go1 envs on a small rough trimesh with the
    height scan, every switch on, noise off: [lin(3) ang(3) world lin(3) ang(3) gravity(3) commands(3) joints(36) yaw(1)
    heights(187)] = 242 entries, the yaw entry between the actions and the heights."""
    from lrl.env import LeggedRobotEnv
    n, no = 64, 55 + 187
    over = dict(ALL_ON, **{"terrain.mesh_type": "trimesh", "terrain.measure_heights": True, "terrain.curriculum": True,
                           "terrain.terrain_proportions": [0.1, 0.1, 0.35, 0.25, 0.2], "terrain.border_size": 3.0,
                           "terrain.teleport_robots": False, "terrain.num_rows": 4, "terrain.num_cols": 4,
                           "terrain.max_init_terrain_level": 3, "env.num_observations": no})
    cfg = _cfg("go1", n, **over)
    env = LeggedRobotEnv("cuda:0", cfg=cfg, seed=5)
    assert env._P.terrain_mesh == 1 and np.abs(env.terrain.heightsamples).max() > 0 and env.num_obs == no
    env.reset()
    rng = np.random.default_rng(41)
    _spin(env, rng)
    seen = np.zeros(3, int)
    for s in range(4):
        env.step(_dev(rng.normal(size=(n, 12)) * 0.5))
        torch.cuda.synchronize()
        h = _assert_rows(env, cfg, what=f"step {s}")
        seen += [np.sum(np.abs(h) <= 2.0), np.sum(h > 2.0), np.sum(h < -2.0)]
        obs = _np(env.obs_buf)
        assert np.abs(obs[:, 55:]).max() > 0 and np.abs(obs[:, 54]).max() == 1.0  # the scan; a clipped yaw entry
        assert np.abs(obs[:, 6:9] - obs[:, 0:3]).max() > 1e-3  # world against base-frame linear velocity
    assert seen.min() > 0, seen  # unclipped, clipped-high and clipped-low headings
    env.close()


@pytest.mark.parametrize("device_resets", [False, True])
def test_reset_path_rows_match_restatement(device_resets):
    """Upstream semantics (legacy_fork=False) with 0.12 s episodes: envs time out inside the step and their rows are
    rebuilt by observe_kernel from the post-reset state; every row (reset in the step or not) equals the restatement
    and the newest history slot equals the row, on the host-list and the device-list reset paths."""
    from lrl.env import LeggedRobotEnv
    from lrl.history import HistoryWrapper
    n, no = 64, 55
    cfg = _cfg("go1", n, **dict(ALL_ON, **{"env.num_observations": no, "env.episode_length_s": 0.12}))
    env = HistoryWrapper(LeggedRobotEnv("cuda:0", cfg=cfg, seed=3, legacy_fork=False, device_resets=device_resets))
    e = env.env
    assert e._dev_path == device_resets and e.max_episode_length == 7  # ceil(0.12 / (4 x float32(0.005)))
    env.reset()
    rng = np.random.default_rng(43)
    _spin(e, rng)
    e.episode_length_buf[:] = _dev(rng.integers(0, 8, n), torch.int32)  # staggered time-outs
    n_reset = 0
    for s in range(5):
        _, _, done, _ = env.step(_dev(rng.normal(size=(n, 12)) * 0.5))
        torch.cuda.synchronize()
        rst = _np(done).astype(bool)
        n_reset += int(rst.sum())
        assert 0 < rst.sum() < n, f"step {s}: {rst.sum()} resets"
        _assert_rows(e, cfg, what=f"step {s}, every env")
        _assert_rows(e, cfg, rows=rst, what=f"step {s}, the envs reset in it")
        np.testing.assert_array_equal(_np(env.obs_history)[:, -no:], _np(e.obs_buf))
        assert np.all(_np(e.episode_length_buf)[rst] == 0)
    assert n_reset >= n // 2
    e.close()


WIDTHS = [45, 49, 55]  # 45 + 18 = 63: one under the 64-float row of the act chain's input; 49: 67, the first past it


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("no", WIDTHS)
def test_fused_policy_act_matches_torch(n, no):
    """test_ppo_gpu.py::test_fused_policy_act_matches_torch at the new observation widths."""
    from lrl.ppo.actor_critic import ActorCritic
    ac = ActorCritic(no, 18, 15 * no, 12).cuda()
    init_params(ac)
    with torch.no_grad():
        ac.std.copy_(torch.linspace(0.5, 1.5, 12))
    g = torch.Generator(device="cuda:0").manual_seed(3)
    obs = torch.randn(n, no, device="cuda:0", generator=g)
    priv = torch.randn(n, 18, device="cuda:0", generator=g)
    eps = torch.randn(n, 12, device="cuda:0", generator=g)
    a, mu, v, lp = ac.act_fused(obs, priv, eps=eps)
    with torch.no_grad():
        ac.update_distribution(obs, priv)
        mu_ref = ac.action_mean
        a_ref = mu_ref + ac.action_std * eps
        lp_ref = ac.get_actions_log_prob(a_ref)
        v_ref = ac.evaluate(obs, priv)
    torch.testing.assert_close(mu, mu_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a, a_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(v, v_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lp, lp_ref, rtol=1e-4, atol=1e-3)


def _random_storage(alg, seed=1):
    st = alg.storage
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    with torch.no_grad():
        for name in ("observations", "privileged_observations", "observation_histories", "actions", "mu"):
            getattr(st, name).copy_(torch.randn(getattr(st, name).shape, device="cuda:0", generator=g))
        st.sigma.fill_(1.0)
        st.values.copy_(torch.randn(st.values.shape, device="cuda:0", generator=g))
        st.returns.copy_(st.values + 0.3 * torch.randn(st.values.shape, device="cuda:0", generator=g))
        a = torch.randn(st.advantages.shape, device="cuda:0", generator=g)
        st.advantages.copy_((a - a.mean()) / a.std())
        st.actions_log_prob.copy_(-11.0 + torch.randn(st.values.shape, device="cuda:0", generator=g))


@pytest.mark.parametrize("mb", [37, 300])
@pytest.mark.parametrize("no", WIDTHS)
def test_native_minibatch_gradients_match_autograd(mb, no):
    """test_ppo_gpu.py::test_native_minibatch_gradients_match_autograd at the new widths: one minibatch of ``mb`` rows
    gathered from a 25 x 12 storage (history rows at the storage's padded pitch), every parameter's gradient, the KL
    mean and the losses against torch autograd of the reference's loss, at that test's bars."""
    from lrl.ppo.actor_critic import ActorCritic
    from lrl.ppo.ppo import PPO, PPO_Args
    N, T = 25, 12
    nh = 15 * no
    ac = ActorCritic(no, 18, nh, 12)
    init_params(ac)
    alg = PPO(ac.cuda(), device="cuda:0", fused=True)
    alg.init_storage(N, T, [no], [18], [nh], [12])
    _random_storage(alg)
    rows = torch.randperm(N * T, device="cuda:0")[:mb].contiguous()
    nst = alg._native_state(mb)
    net, hp, grads, ctrl, ws = nst["net"], nst["hp"], nst["grads"], nst["ctrl"], nst["ws"]
    s = alg.storage
    fl = lambda t: t.flatten(0, 1)
    batch = _abi.LrlPpoBatch()
    for k, t in dict(obs=s.observations, priv=s.privileged_observations, hist=s.observation_histories,
                     actions=s.actions, values=s.values, returns=s.returns, logp=s.actions_log_prob,
                     adv=s.advantages, mu=s.mu, sigma=s.sigma).items():
        setattr(batch, k, fl(t).data_ptr())
    batch.rows, batch.batch = rows.data_ptr(), mb
    hist_flat = fl(s.observation_histories)
    assert hist_flat.stride(0) == (nh + 15) // 16 * 16
    batch.hist_ld = hist_flat.stride(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _abi.lib()
    _abi.check(L.lrl_ppo_forward_backward(C.byref(net), p(ac._flat), p(grads), C.byref(batch), C.byref(hp), p(ws),
                                          p(ctrl), stream))
    _abi.check(L.lrl_ppo_adaptation_forward_backward(C.byref(net), p(ac._flat), None, p(grads), C.byref(batch),
                                                     p(ws), p(ctrl), stream))
    torch.cuda.synchronize()
    mbf = ctrl.view(torch.float32)[8:12].tolist()  # value, surrogate, adaptation, (kl in grads)
    kl_native = grads[net.kl_slot].item()
    b = tuple(fl(t)[rows] for t in (s.observations, s.actions, s.values, s.returns, s.actions_log_prob, s.advantages,
                                    s.mu, s.sigma))
    ref = autograd_minibatch(ac, PPO_Args, b, torch.float32, priv=fl(s.privileged_observations)[rows],
                             hist=fl(s.observation_histories)[rows])
    np.testing.assert_allclose(kl_native, ref.kl, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(mbf[:3], [ref.value_loss, ref.surrogate, ref.adaptation_loss], rtol=1e-4, atol=1e-7)
    bad = []
    for name, prm in ac.named_parameters():
        off = (prm.data_ptr() - ac._flat.data_ptr()) // 4
        got = grads[off:off + prm.numel()].view_as(prm)
        r = ref.grads[name]
        err = (got - r).abs().max().item()
        if not err <= 1e-4 * (r.abs().max().item() + 1e-6) + 1e-7:
            bad.append(f"{name}: err {err:.3g} ref max {r.abs().max().item():.3g} got max {got.abs().max().item():.3g}")
    assert not bad, "\n".join(bad)


def test_runner_learns_at_width_55():
    """One Runner.learn iteration over HistoryWrapper at 64 envs with every switch on: the 55-wide rows reach the
    native act / update, finite losses and parameters."""
    from lrl.env import LeggedRobotEnv
    from lrl.history import HistoryWrapper
    from lrl.ppo import runner as R
    n = 64
    cfg = _cfg("go1", n, **dict(ALL_ON, **{"env.num_observations": 55}))
    R.RunnerArgs.save_interval = 0
    env = HistoryWrapper(LeggedRobotEnv("cuda:0", cfg=cfg, seed=2, legacy_fork=False))
    assert env.num_obs == 55 and env.num_obs_history == 15 * 55
    runner = R.Runner(env, device="cuda:0", seed=2)
    losses, update = [], runner.alg.update
    runner.alg.update = lambda *a, **k: losses.append(update(*a, **k)) or losses[-1]
    runner.learn(1, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert len(losses) == 1 and all(np.isfinite(float(x)) for x in losses[0]), losses  # value, surrogate, adaptation
    st = runner.alg.storage
    assert tuple(st.observations.shape[-1:]) == (55,) and tuple(_np(env.env.obs_buf).shape) == (n, 55)
    assert np.isfinite(_np(env.env.obs_buf)).all()
    assert torch.isfinite(st.observations).all() and torch.isfinite(st.values).all() and torch.isfinite(st.actions).all()
    assert torch.isfinite(runner.alg.actor_critic._flat).all()
    env.env.close()
