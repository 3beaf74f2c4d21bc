"""Generate the high-level policy's PPO fixtures by RUNNING the reference's own ``high_level_policy.ppo``.

IN-CONTAINER ONLY, like ``make_golden.py`` (whose stubs, ``init_params`` and paths this imports): nothing here runs on
the GPU box, and no reference source is copied.  Every random draw (Normal samples, the minibatch permutation) is
injected and recorded.

Fixtures written:
  hlp_ppo_update.npz         PPO.act / process_env_step / compute_returns / update (high_level_policy/ppo/ppo.py) of
                             the plain tanh actor-critic (USE_LATENT = False): 14 obs, 18 privileged, 16 history,
                             3 actions; N = 19 envs x T = 20 steps, so a minibatch is 95 rows — no multiple of 4, 16
                             or 64.
  hlp_state_dict_keys.json   the ActorCritic's state-dict layout (17 keys: actor_body, critic_body, std)

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hlp.py
"""
import json
import os

import numpy as np
import torch

from make_golden import HERE, init_params  # (installs the reference's import stubs and puts it on sys.path)

NO, NP, NH, NA = 14, 18, 16, 3
N, T = 19, 20


def gen_hlp_ppo():
    import high_level_policy
    from high_level_policy.ppo.actor_critic import ActorCritic
    from high_level_policy.ppo.ppo import PPO

    assert high_level_policy.USE_LATENT is False
    torch.manual_seed(0)
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)  # (std = ones)
    sd_keys = [(k, list(v.shape)) for k, v in ac.state_dict().items()]
    with open(os.path.join(HERE, "hlp_state_dict_keys.json"), "w") as f:
        json.dump(sd_keys, f, indent=0)
    params0 = {k: v.detach().clone() for k, v in ac.named_parameters()}

    alg = PPO(ac, device="cpu")
    alg.init_storage(N, T, [NO], [NP], [NH], [NA])
    rng = np.random.default_rng(43)
    q = lambda a: (np.round(a * 64) / 64).astype(np.float32)  # multiples of 1/64: exact in fp32, compressible
    obs_seq = q(rng.normal(size=(T + 1, N, NO)))
    priv_seq = q(rng.normal(size=(T + 1, N, NP)))
    hist_seq = q(rng.normal(size=(T + 1, N, NH)))
    eps = q(rng.normal(size=(T, N, NA)))
    rew = rng.normal(size=(T, N)).astype(np.float32) * 0.1
    done = rng.random((T, N)) < 0.05
    perm = rng.permutation(T * N)
    actions_rec, values_rec, logp_rec, mu_rec = [], [], [], []
    orig_sample = torch.distributions.Normal.sample
    try:
        for t in range(T):
            def fake_sample(self, sample_shape=torch.Size(), _t=t):
                return self.mean + self.stddev * torch.tensor(eps[_t])
            torch.distributions.Normal.sample = fake_sample
            with torch.inference_mode():
                a = alg.act(torch.tensor(obs_seq[t]), torch.tensor(priv_seq[t]), torch.tensor(hist_seq[t]))
                actions_rec.append(a.numpy().copy())
                values_rec.append(alg.transition.values.numpy().copy())
                logp_rec.append(alg.transition.actions_log_prob.numpy().copy())
                mu_rec.append(alg.transition.action_mean.numpy().copy())
                alg.process_env_step(torch.tensor(rew[t]), torch.tensor(done[t]), {})  # (no env_bins, no time_outs)
    finally:
        torch.distributions.Normal.sample = orig_sample
    with torch.inference_mode():
        alg.compute_returns(torch.tensor(obs_seq[T]), torch.tensor(priv_seq[T]))
    returns = alg.storage.returns.numpy().copy()
    adv = alg.storage.advantages.numpy().copy()

    lrs = []
    orig_randperm = torch.randperm
    torch.randperm = lambda n, **kw: torch.tensor(perm)
    orig_step = alg.optimizer.step

    def step_rec(*a, **k):
        lrs.append(alg.learning_rate)
        return orig_step(*a, **k)
    alg.optimizer.step = step_rec
    try:
        mv, ms_, ma = alg.update()
    finally:
        torch.randperm = orig_randperm
    params1 = {k: v.detach().numpy().copy() for k, v in ac.named_parameters()}
    out = dict(obs_seq=obs_seq, priv_seq=priv_seq, hist_seq=hist_seq, eps=eps, rew=rew, done=done.astype(np.uint8),
               perm=perm, actions=np.stack(actions_rec), values=np.stack(values_rec), logp=np.stack(logp_rec),
               mu=np.stack(mu_rec), returns=returns, advantages=adv, lrs=np.array(lrs),
               mean_value_loss=np.array(mv), mean_surrogate_loss=np.array(ms_), mean_adaptation_loss=np.array(ma))
    names = sorted(params1)
    out["param_names"] = np.array(names)
    out["param_sums"] = np.array([params1[k].astype(np.float64).sum() for k in names])
    out["param_abs_sums"] = np.array([np.abs(params1[k].astype(np.float64)).sum() for k in names])
    out["param_delta_norm"] = np.array([np.linalg.norm((params1[k] - params0[k].numpy()).astype(np.float64))
                                        for k in names])
    out["param_head"] = np.stack([np.pad(params1[k].ravel()[:16], (0, max(0, 16 - params1[k].size)))
                                  for k in names])
    np.savez_compressed(os.path.join(HERE, "hlp_ppo_update.npz"), **out)
    print("hlp ppo: keys", len(sd_keys), "lr", lrs[:4], "losses", mv, ms_, ma)


if __name__ == "__main__":
    gen_hlp_ppo()
