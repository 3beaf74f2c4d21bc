"""Runner.learn with the history shift done by the act (PPO.act(shift_history=True) + env.history_preshifted, the
default) against the same run with LRL_ACT_SHIFT_HISTORY=0 (the env's step shifts every row): two iterations on the
Mini Cheetah preset with fresh envs and runners made alike; the rollout storage, the env's history and observations and
the policy parameters must be the same bits.

256 train envs is in the GEMM chain's row range (64 to 2047: act_head_kernel does the shift); the same run with
LRL_ACT_FUSED=1 takes the one-launch act (act_fused_kernel does it); with eval envs present (192 + 64) the act shifts
the train rows and the sim's shift launch the eval rows.  The switch is read by each learn call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cfg(n):
    from lrl import config as lcfg
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = n
    return cfg


def _run(n_train, n_eval, shift, monkeypatch):
    from lrl.env import LeggedRobotEnv
    from lrl.history import HistoryWrapper
    from lrl.ppo import runner as R
    monkeypatch.setattr(R.RunnerArgs, "save_interval", 0)
    monkeypatch.setattr(R.RunnerArgs, "log_freq", 10 ** 9)
    monkeypatch.setenv("LRL_ACT_SHIFT_HISTORY", shift)
    torch.manual_seed(0)
    env = HistoryWrapper(LeggedRobotEnv(DEV, cfg=_cfg(n_train), eval_cfg=_cfg(n_eval) if n_eval else None, seed=1234))
    calls = []
    told = env.env.history_preshifted
    env.env.history_preshifted = lambda rows: (calls.append(rows), told(rows))[1]
    try:
        runner = R.Runner(env, device=DEV, seed=1234)
        assert runner.alg.fused
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        st = runner.alg.storage
        # (every array of the storage; its private scratch — the update's workspace — holds no result)
        out = {"storage/" + k: v.clone() for k, v in vars(st).items()
               if isinstance(v, torch.Tensor) and not k.startswith("_")}
        assert {"storage/observation_histories", "storage/observations", "storage/actions", "storage/rewards"} <= set(out)
        e = env.env
        out.update(history=e.obs_history_buf.clone(), obs=e.obs_buf.clone(), priv=e.privileged_obs_buf.clone(),
                   root=e.root_states.clone(), dof_pos=e.dof_pos.clone(),
                   params=runner.alg.actor_critic._flat.detach().clone())
        steps = 2 * runner.num_steps_per_env
    finally:
        env.env.close()
    return out, calls, steps


@pytest.mark.parametrize("n_train,n_eval,fused", [(256, 0, None), (256, 0, "1"), (192, 64, None)],
                         ids=["chain", "one-launch", "eval-envs"])
def test_learn_is_the_same_with_the_shift_in_the_act(n_train, n_eval, fused, monkeypatch):
    if fused is None:
        monkeypatch.delenv("LRL_ACT_FUSED", raising=False)
    else:
        monkeypatch.setenv("LRL_ACT_FUSED", fused)
    on, calls_on, steps = _run(n_train, n_eval, "1", monkeypatch)
    off, calls_off, _ = _run(n_train, n_eval, "0", monkeypatch)
    assert calls_on == [n_train] * steps, "the rollout did not ask the act for the shift at every step"
    assert calls_off == []
    assert set(on) == set(off)
    for k in on:
        a, b = on[k], off[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        else:
            assert torch.equal(a, b), k
    h = on["history"]
    assert torch.isfinite(h).all() and (h[:, -42:] != 0).any()
    assert torch.equal(h[:, -42:], on["obs"])  # the newest slot is the step's observation, in every row
