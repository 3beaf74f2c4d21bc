"""The high-level (navigation) policy's learning side on the CPU: the reference's import paths, the 17-key plain tanh
actor-critic, and the torch-autograd PPO (fused=False) against the reference's own run
(tests/golden/hlp_ppo_update.npz, written by tests/golden/make_golden_hlp.py)."""
import json
import os
import zlib

import numpy as np
import torch

from helpers import GOLDEN, golden

NO, NP, NH, NA = 14, 18, 16, 3


def init_params(module):
    """Same deterministic init as tests/golden/make_golden.py::init_params."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            r = np.random.default_rng(zlib.crc32(name.encode()))
            fan_in = p.shape[-1] if p.dim() > 1 else 1
            scale = 1.0 / np.sqrt(fan_in) if p.dim() > 1 else 0.05
            if name == "std":
                p.copy_(torch.ones_like(p))
            else:
                p.copy_(torch.tensor(r.uniform(-1, 1, tuple(p.shape)) * scale, dtype=torch.float))


def test_reference_import_paths_resolve():
    import high_level_policy
    import high_level_policy.ppo as P
    from high_level_policy.ppo.actor_critic import AC_Args, ActorCritic
    from high_level_policy.ppo.ppo import PPO, PPO_Args
    from high_level_policy.ppo.rollout_storage import RolloutStorage
    import lrl.hlp as H
    assert high_level_policy.USE_LATENT is False and os.path.isdir(high_level_policy.HLP_ROOT_DIR)
    assert P.Runner is H.Runner and P.RunnerArgs is H.RunnerArgs and P.ActorCritic is ActorCritic is H.ActorCritic
    assert P.RolloutStorage is RolloutStorage is H.RolloutStorage and PPO is H.PPO and PPO_Args is H.PPO_Args
    assert hasattr(P.caches, "slot_cache") and hasattr(P.caches, "dist_cache")
    assert AC_Args.activation == "tanh" and AC_Args.actor_hidden_dims == [512, 256, 128]
    assert AC_Args.critic_hidden_dims == [512, 256, 128] and AC_Args.init_noise_std == 1.0
    assert P.RunnerArgs.num_steps_per_env == 200 and P.RunnerArgs.max_iterations == 1500
    assert P.RunnerArgs.save_interval == 400 and P.RunnerArgs.log_freq == 10
    ref = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01,
               num_learning_epochs=5, num_mini_batches=4, learning_rate=1.e-3, adaptation_module_learning_rate=1.e-3,
               num_adaptation_module_substeps=1, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01,
               max_grad_norm=1.)
    assert {k: getattr(PPO_Args, k) for k in ref} == ref
    # the low-level argument classes are separate objects: changing one policy's arguments leaves the other's alone
    from lrl.ppo.ppo import PPO_Args as LL_Args
    from lrl.ppo.runner import RunnerArgs as LL_RunnerArgs
    assert PPO_Args is not LL_Args and P.RunnerArgs is not LL_RunnerArgs and LL_RunnerArgs.num_steps_per_env == 24


def test_state_dict_layout_matches_reference():
    from lrl.hlp import ActorCritic
    with open(os.path.join(GOLDEN, "hlp_state_dict_keys.json")) as f:
        want = [(k, list(s)) for k, s in json.load(f)]
    ac = ActorCritic(NO, NP, NH, NA)
    got = [(k, list(v.shape)) for k, v in ac.state_dict().items()]
    assert len(got) == 17 and got == want
    assert isinstance(ac.actor_body[1], torch.nn.Tanh) and isinstance(ac.critic_body[1], torch.nn.Tanh)


def test_low_level_actor_critic_keeps_its_35_keys():
    from lrl.ppo.actor_critic import ActorCritic
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        want = [(k, list(s)) for k, s in json.load(f)]
    got = [(k, list(v.shape)) for k, v in ActorCritic(42, 18, 630, 12).state_dict().items()]
    assert len(got) == 35 and got == want


def test_privileged_and_history_inputs_are_ignored():
    from lrl.hlp import ActorCritic
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)
    g = torch.Generator().manual_seed(2)
    obs, priv, hist = torch.randn(5, NO, generator=g), torch.randn(5, NP, generator=g), torch.randn(5, NH, generator=g)
    with torch.no_grad():
        mean = ac.actor_body(obs)
        assert torch.equal(ac.act_teacher(obs, priv), mean) and torch.equal(ac.act_student(obs, hist), mean)
        ob = dict(obs=obs, privileged_obs=priv, obs_history=hist)
        assert torch.equal(ac.act_inference(ob), mean) and torch.equal(ac.act_expert(ob), mean)
        assert torch.equal(ac.evaluate(obs, priv), ac.critic_body(obs))
        ac.act(obs, priv)
        assert torch.equal(ac.action_mean, mean) and torch.equal(ac.action_std, torch.ones(5, NA))


def test_flat_parameter_descriptor_is_plain_tanh():
    from lrl.hlp import ActorCritic
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    net = ac.flatten_parameters()
    assert (net.plain, net.activation, net.latent, net.enc_h0, net.enc_h1, net.ad_h0, net.ad_h1) == (1, 1, 0, 0, 0, 0, 0)
    assert (net.num_obs, net.num_priv, net.num_hist, net.num_actions) == (NO, NP, NH, NA)
    assert (net.ac_h0, net.ac_h1, net.ac_h2) == (512, 256, 128) and net.adapt_begin == net.adapt_end
    offs = [net.w1, net.b1, net.w2, net.b2, net.w3, net.b3, net.w4a, net.b4a, net.w4c, net.b4c, net.std_off]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs) and net.main_begin == 0
    assert net.main_end == net.kl_slot == net.std_off + NA and net.kl_slot < net.total == ac._flat.numel()
    for k, v in ac.state_dict().items():  # the tensors are views of the flat buffer and kept their values
        assert torch.equal(v, before[k])
        assert ac._flat.data_ptr() <= v.data_ptr() < ac._flat.data_ptr() + 4 * net.total
    # [actor; critic] pairs adjacent: the critic's layer follows the actor's
    a1, c1 = ac.actor_body[0].weight, ac.critic_body[0].weight
    assert c1.data_ptr() == a1.data_ptr() + 4 * a1.numel() == ac._flat.data_ptr() + 4 * (net.w1 + 512 * NO)


def test_torch_ppo_reproduces_reference_rollout_gae_update():
    """PPO.act -> process_env_step (infos without env_bins) -> returns -> update on the torch-autograd path against the
    reference's run: the comparisons and bars of test_ppo_rollout_gae_update_match_reference.  (The storage's GAE is a
    HIP kernel; here the oracle's numpy GAE fills returns / advantages from what the rollout stored.)"""
    from lrl.hlp import PPO, ActorCritic
    from oracle import oracle
    g = golden("hlp_ppo_update.npz")
    T, N = g["eps"].shape[:2]
    assert (T, N) == (20, 19) and g["eps"].shape[2] == NA
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)
    alg = PPO(ac, device="cpu", fused=False)
    alg.init_storage(N, T, [NO], [NP], [NH], [NA])
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    orig_sample = torch.distributions.Normal.sample
    try:
        for t in range(T):
            torch.distributions.Normal.sample = (
                lambda self, sample_shape=torch.Size(), _t=t: self.mean + self.stddev * d(g["eps"][_t]))
            with torch.inference_mode():
                a = alg.act(d(g["obs_seq"][t]), d(g["priv_seq"][t]), d(g["hist_seq"][t]))
                np.testing.assert_allclose(a.numpy(), g["actions"][t], rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(alg.transition.values.numpy(), g["values"][t], rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(alg.transition.actions_log_prob.numpy(), g["logp"][t], rtol=1e-4, atol=2e-4)
                alg.process_env_step(d(g["rew"][t]), d(g["done"][t]).bool(), {})
    finally:
        torch.distributions.Normal.sample = orig_sample
    s = alg.storage
    with torch.inference_mode():
        last = ac.evaluate(d(g["obs_seq"][T]), d(g["priv_seq"][T]))
    ret, adv = oracle.gae(s.rewards.numpy(), s.dones.numpy(), s.values.numpy(), last.numpy(), PPO.args.gamma,
                          PPO.args.lam)
    np.testing.assert_allclose(ret, g["returns"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(adv, g["advantages"], rtol=1e-4, atol=1e-4)
    s.returns.copy_(d(ret))
    s.advantages.copy_(d(adv.astype(np.float32)))
    np.testing.assert_array_equal(s.observation_histories.numpy(), g["hist_seq"][:T])
    np.testing.assert_array_equal(s.privileged_observations.numpy(), g["priv_seq"][:T])
    lrs = []
    orig_step = alg.optimizer.step
    alg.optimizer.step = lambda *a, **k: (lrs.append(alg.learning_rate), orig_step(*a, **k))[1]
    perm = d(g["perm"])
    orig = torch.randperm
    torch.randperm = lambda n, **kw: perm
    try:
        mv, ms, ma = alg.update()
    finally:
        torch.randperm = orig
    assert ma == 0 and float(g["mean_adaptation_loss"]) == 0
    np.testing.assert_allclose(lrs, g["lrs"], rtol=1e-9)
    np.testing.assert_allclose([mv, ms], [g["mean_value_loss"], g["mean_surrogate_loss"]], rtol=2e-3, atol=1e-5)
    params = dict(ac.named_parameters())
    names = [str(x) for x in g["param_names"]]
    assert sorted(params) == names
    sums = np.array([params[k].detach().double().sum().item() for k in names])
    np.testing.assert_allclose(sums, g["param_sums"], rtol=2e-3, atol=2e-3)
    heads = np.stack([np.pad(params[k].detach().numpy().ravel()[:16], (0, max(0, 16 - params[k].numel())))
                      for k in names])
    np.testing.assert_allclose(heads, g["param_head"], rtol=2e-3, atol=1e-4)


def test_metric_caches_keep_running_means():
    from high_level_policy.ppo.metrics_caches import DistCache, SlotCache
    dc = DistCache()
    dc.log(x=np.ones(3))
    dc.log(x=np.zeros(3))
    np.testing.assert_array_equal(dc.get_summary()["x"], 0.5 * np.ones(3))
    assert dc.get_summary() == {}
    sc = SlotCache(5)
    sc.log([1, 3], v=[2.0, 4.0])
    sc.log([1], v=[4.0])
    sc.log(v=np.ones(5))
    np.testing.assert_allclose(sc.get_summary()["v"], [1.0, (2 + 4 + 1) / 3, 1.0, (4 + 1) / 2, 1.0])
