"""The high-level (navigation) policy's native learning path on the GPU: the tanh GEMM epilogues, the plain-form
act / forward-backward / update of csrc/lrl_ppo.hip (14 observations, 3 actions, no latent), and one Runner.learn
iteration over HighLevelControlWrapper."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest
import torch

from helpers import GOLDEN, autograd_minibatch, golden
from lrl import _abi

pytestmark = pytest.mark.gpu
dev = "cuda:0"
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


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gemm_rc(layout, epi, M, N, K, A, lda, B, ldb, Cm, ldc, bias=None, aux=None, ld_aux=0, planes=False):
    """lrl_gemm_f32's return code.  planes: B pre-split into bf16 planes (layout | 0x100), which runs the product on
    the pre-split-B kernel or fails."""
    ws = torch.empty(3 * N * ((K + 15) // 16 * 16) // 2 + 64, device=dev) if planes else None
    rc = _abi.lib().lrl_gemm_f32(C.c_int32(layout | (0x100 if planes else 0)), C.c_int32(epi), C.c_int32(M),
                                 C.c_int32(N), C.c_int32(K), _p(A), C.c_int64(lda), _p(B), C.c_int64(ldb), _p(Cm),
                                 C.c_int64(ldc), _p(bias), _p(aux), C.c_int64(ld_aux), None, _p(ws),
                                 C.c_int64(ws.numel() if planes else 0), _stream())
    torch.cuda.synchronize()
    return rc


# ---- 1. the tanh epilogues through lrl_gemm_f32 --------------------------------------------------------------
# The bar is relative to torch's own fp32 error on the same inputs: both are measured against a float64 evaluation, and
# the native error may be at most twice torch's (another summation order, another tanh).  The ratios print with -s.
# (300, 24, 512) takes the thin kernel; planes: the pre-split-B kernel
@pytest.mark.parametrize("M,N,K,planes", [(95, 1024, 16, False), (185, 256, 512, False), (4096, 128, 256, False),
                                          (300, 24, 512, False), (4096, 128, 256, True)])
def test_bias_tanh_epilogue_against_float64(M, N, K, planes):
    g = torch.Generator(device=dev).manual_seed(M + 3 * N + K)
    X = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) / np.sqrt(K)
    b = torch.randn(N, device=dev, generator=g)
    ref = torch.tanh(X.double() @ W.double().T + b.double())
    t32 = torch.tanh(X @ W.T + b)
    out = torch.full((M, N), float("nan"), device=dev)
    assert _gemm_rc(0, 5, M, N, K, X, K, W, K, out, N, bias=b, planes=planes) == 0
    assert torch.isfinite(out).all()
    e_nat, e_t32 = (out.double() - ref).abs().max().item(), (t32.double() - ref).abs().max().item()
    print(f"epi5 {M}x{N}x{K}{' planes' if planes else ''}: native {e_nat:.3e} torch-fp32 {e_t32:.3e} ratio {e_nat / e_t32:.2f}")
    assert e_nat <= 2.0 * e_t32


@pytest.mark.parametrize("M,N,K,planes", [(185, 512, 256, False), (95, 16, 1024, False), (192, 512, 256, True)])
def test_dtanh_epilogue_against_float64(M, N, K, planes):
    g = torch.Generator(device=dev).manual_seed(M + 5 * N + K)
    dY = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(K, N, device=dev, generator=g) / np.sqrt(K)
    H = torch.tanh(torch.randn(M, N, device=dev, generator=g))  # the layer input: a tanh output
    ref = (dY.double() @ W.double()) * (1.0 - H.double() ** 2)
    t32 = (dY @ W) * (1.0 - H * H)
    out = torch.full((M, N), float("nan"), device=dev)
    assert _gemm_rc(2, 6, M, N, K, dY, K, W, N, out, N, aux=H, ld_aux=N, planes=planes) == 0
    assert torch.isfinite(out).all()
    e_nat, e_t32 = (out.double() - ref).abs().max().item(), (t32.double() - ref).abs().max().item()
    print(f"epi6 {M}x{N}x{K}{' planes' if planes else ''}: native {e_nat:.3e} torch-fp32 {e_t32:.3e} ratio {e_nat / e_t32:.2f}")
    assert e_nat <= 2.0 * e_t32


def test_tanh_epilogue_keeps_relative_accuracy_near_zero():
    """Pre-activations inside +-1e-3, formed without cancellation (every product and bias of a column has the column's
    sign), so the relative error of the output is the relative error of the sum plus tanh's own: a tanh evaluated as
    1 - 2 / (exp(2x) + 1) is off by ~6e-8 absolute there, 1e-4 relative, and fails both bars.  The a-priori bar:
    K products and K additions at 2^-24 each, the bias addition, and 4 ulp for tanh itself."""
    M, N, K = 95, 256, 16
    g = torch.Generator(device=dev).manual_seed(11)
    X = torch.rand(M, K, device=dev, generator=g)
    sign = torch.where(torch.arange(N, device=dev) % 2 == 0, 1.0, -1.0)
    W = torch.rand(N, K, device=dev, generator=g) * 5e-5 * sign[:, None]
    b = torch.rand(N, device=dev, generator=g) * 2e-4 * sign
    pre = X.double() @ W.double().T + b.double()
    assert pre.abs().max().item() < 1e-3 and pre.abs().min().item() > 1e-6
    ref = torch.tanh(pre)
    t32 = torch.tanh(X @ W.T + b)
    out = torch.full((M, N), float("nan"), device=dev)
    assert _gemm_rc(0, 5, M, N, K, X, K, W, K, out, N, bias=b) == 0
    r_nat = ((out.double() - ref).abs() / ref.abs()).max().item()
    r_t32 = ((t32.double() - ref).abs() / ref.abs()).max().item()
    print(f"epi5 near zero: native rel {r_nat:.3e} torch-fp32 rel {r_t32:.3e} ratio {r_nat / r_t32:.2f}")
    assert r_nat <= 2.0 * r_t32
    assert r_nat <= (2 * K + 1 + 4) * 2.0 ** -24


def test_tanh_epilogues_refuse_the_other_layouts():
    """epi 5 is a forward (NT) epilogue and epi 6 a backward-data (NN) one: any other pairing is an error, never the ELU
    instantiation a launcher would otherwise default to; the output stays untouched."""
    M = N = K = 64
    A = torch.randn(M, K, device=dev)
    B = torch.randn(N, K, device=dev)
    b = torch.randn(N, device=dev)
    for layout, epi in ((2, 5), (0, 6), (3, 5), (3, 6)):
        out = torch.full((M, N), 7.0, device=dev)
        assert _gemm_rc(layout, epi, M, N, K, A, K, B, K, out, N, bias=b, aux=A, ld_aux=K) != 0
        assert (out == 7.0).all()
    out = torch.full((M, N), 7.0, device=dev)
    assert _gemm_rc(2, 6, M, N, K, A, K, B, N, out, N, aux=None) != 0 and (out == 7.0).all()  # epi 6 needs aux


# ---- 2. the plain-form act ------------------------------------------------------------------------------------
def _hlp_ac(std=None):
    from lrl.hlp import ActorCritic
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)
    ac = ac.cuda()
    if std is not None:
        with torch.no_grad():
            ac.std.copy_(torch.as_tensor(std, device=dev))
    return ac


@pytest.mark.parametrize("n", [37, 972])
def test_plain_act_matches_torch(n):
    """lrl_ppo_act on the plain tanh net (priv = hist = NULL) against the torch module, eps injected: the bars of
    test_fused_policy_act_matches_torch."""
    ac = _hlp_ac(std=[0.5, 1.0, 1.5])
    g = torch.Generator(device=dev).manual_seed(3)
    obs = torch.randn(n, NO, device=dev, generator=g)
    eps = torch.randn(n, NA, device=dev, generator=g)
    a, mu, v, lp = ac.act_fused(obs, None, eps=eps)
    torch.cuda.synchronize()
    with torch.no_grad():
        ac.update_distribution(obs, None)
        mu_ref = ac.action_mean
        a_ref = mu_ref + ac.action_std * eps
        lp_ref = ac.get_actions_log_prob(a_ref)
        v_ref = ac.evaluate(obs, None)
    torch.testing.assert_close(mu, mu_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a, a_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(v, v_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lp, lp_ref, rtol=1e-4, atol=1e-3)


def test_plain_act_writes_the_storage_row():
    from lrl.hlp import RolloutStorage
    n = 37
    ac = _hlp_ac(std=[0.5, 1.0, 1.5])
    g = torch.Generator(device=dev).manual_seed(5)
    obs, priv, hist = (torch.randn(n, k, device=dev, generator=g) for k in (NO, NP, NH))
    st = RolloutStorage(n, 3, [NO], [NP], [NH], [NA], dev)
    a, mu, v, lp = ac.act_fused(obs, priv, hist, seed=11, counter=3, store=st.store_desc(), store_row=1)
    a2, mu2, v2, lp2 = ac.act_fused(obs, None, seed=11, counter=3)  # the same draws without the optional inputs
    torch.cuda.synchronize()
    for x, y in ((a, a2), (mu, mu2), (v, v2), (lp, lp2)):
        assert torch.equal(x, y)
    assert torch.equal(st.observations[1], obs) and torch.equal(st.privileged_observations[1], priv)
    assert torch.equal(st.observation_histories[1], hist) and torch.equal(st.actions[1], a)
    assert torch.equal(st.mu[1], mu) and torch.equal(st.values[1], v) and torch.equal(st.actions_log_prob[1, :, 0], lp)
    assert torch.equal(st.sigma[1], ac.std.detach().expand(n, NA))
    for t in (0, 2):  # the other rows stay zero
        assert not st.observations[t].any() and not st.actions[t].any() and not st.values[t].any()
    z = (a - mu) / ac.std.detach()
    assert abs(z.mean().item()) < 0.35 and 0.6 < z.std().item() < 1.4  # (111 counter-RNG normal draws)


# ---- 3. one minibatch of forward_backward against autograd -----------------------------------------------------
def _random_storage(alg, seed=1):
    st = alg.storage
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda t: torch.randn(t.shape, device=dev, generator=g)
    with torch.no_grad():
        for name in ("observations", "privileged_observations", "observation_histories", "actions", "mu"):
            getattr(st, name).copy_(rn(getattr(st, name)))
        st.sigma.fill_(1.0)
        st.values.copy_(rn(st.values))
        st.returns.copy_(st.values + 0.3 * rn(st.values))
        a = rn(st.advantages)
        st.advantages.copy_((a - a.mean()) / a.std())
        # old log-probs near the current policy's (3 actions, unit std) so the ratio straddles the clip range
        st.actions_log_prob.copy_(-4.3 + rn(st.values))


def _autograd_minibatch(ac, args, b, dtype):
    """The reference's loss (ppo.py:104-146) on one minibatch in `dtype`: (kl, value loss, surrogate, {name: grad});
    the restatement itself is helpers.autograd_minibatch."""
    r = autograd_minibatch(ac, args, b, dtype)
    return r.kl, r.value_loss, r.surrogate, r.grads


@pytest.mark.parametrize("N,T", [(37, 20), (972, 200)])
def test_plain_minibatch_gradients_match_autograd(N, T):
    """One minibatch of lrl_ppo_forward_backward on the plain tanh net against torch autograd of the reference's loss:
    every parameter's gradient, the KL mean, both losses — the formula and bars of
    test_native_minibatch_gradients_match_autograd.  mb = 185 rows, and the training script's 972 x 200 / 4 = 48,600;
    neither is a multiple of 64.  The errors of the native result and of torch-fp32 against float64 autograd print
    with -s."""
    from lrl.hlp import PPO
    ac = _hlp_ac()
    alg = PPO(ac, device=dev, fused=True)
    alg.init_storage(N, T, [NO], [NP], [NH], [NA])
    _random_storage(alg)
    mb = N * T // 4
    assert mb % 64 != 0
    rows = torch.randperm(N * T, device=dev, generator=torch.Generator(device=dev).manual_seed(7))[:mb].contiguous()
    nst = alg._native_state(mb)
    net, hp, grads, ctrl, ws = nst["net"], nst["hp"], nst["grads"], nst["ctrl"], nst["ws"]
    assert net.plain == 1 and net.activation == 1
    s = alg.storage
    fl = lambda t: t.flatten(0, 1)
    batch = _abi.LrlPpoBatch()
    for k, t in dict(obs=s.observations, priv=s.privileged_observations, hist=s.observation_histories,
                     actions=s.actions, values=s.values, returns=s.returns, logp=s.actions_log_prob,
                     adv=s.advantages, mu=s.mu, sigma=s.sigma).items():
        setattr(batch, k, fl(t).data_ptr())
    batch.rows, batch.batch, batch.hist_ld = rows.data_ptr(), mb, NH
    grads.fill_(float("nan"))
    _abi.check(_abi.lib().lrl_ppo_forward_backward(C.byref(net), _p(ac._flat), _p(grads), C.byref(batch), C.byref(hp),
                                                   _p(ws), _p(ctrl), _stream()))
    torch.cuda.synchronize()
    mbf = ctrl.view(torch.float32)[8:12].tolist()  # value, surrogate, (adaptation), (kl in grads)
    kl_native = grads[net.kl_slot].item()
    b = tuple(fl(t)[rows] for t in (s.observations, s.actions, s.values, s.returns, s.actions_log_prob, s.advantages,
                                    s.mu, s.sigma))
    kl, vl, surr, g32 = _autograd_minibatch(ac, PPO.args, b, torch.float32)
    _, _, _, g64 = _autograd_minibatch(ac, PPO.args, b, torch.float64)
    fg = grads
    bad = []
    for name, prm in ac.named_parameters():
        off = (prm.data_ptr() - ac._flat.data_ptr()) // 4
        got = fg[off:off + prm.numel()].view_as(prm)
        ref = g32[name]
        err = (got - ref).abs().max().item()
        e_nat = (got.double() - g64[name]).abs().max().item()
        e_t32 = (ref.double() - g64[name]).abs().max().item()
        print(f"mb {mb} {name}: |native - fp32| {err:.3e} (ref max {ref.abs().max().item():.3e}); vs float64: native "
              f"{e_nat:.3e} torch-fp32 {e_t32:.3e}")
        if not err <= 1e-4 * (ref.abs().max().item() + 1e-6) + 1e-7:
            bad.append(f"{name}: err {err:.3g} ref max {ref.abs().max().item():.3g} got max {got.abs().max().item():.3g}")
    print(f"mb {mb}: kl {kl_native:.8e} / {kl:.8e}, value {mbf[0]:.8e} / {vl:.8e}, surrogate {mbf[1]:.8e} / {surr:.8e}")
    np.testing.assert_allclose(kl_native, kl, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(mbf[:2], [vl, surr], rtol=1e-4, atol=1e-7)
    assert not bad, "\n".join(bad)


# ---- 4. the whole fixture on the native path ------------------------------------------------------------------
def test_native_rollout_gae_update_match_reference():
    """PPO.act (native) -> process_env_step (infos without env_bins) -> compute_returns (HIP GAE) -> update (native),
    against the reference's run on the same weights / inputs / noise / permutation (tests/golden/hlp_ppo_update.npz):
    the comparisons and bars of test_ppo_rollout_gae_update_match_reference."""
    from lrl.hlp import PPO
    g = golden("hlp_ppo_update.npz")
    T, N = g["eps"].shape[:2]
    ac = _hlp_ac()
    alg = PPO(ac, device=dev)
    assert alg.fused and not alg.overlap_adaptation
    alg.init_storage(N, T, [NO], [NP], [NH], [NA])
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    with torch.inference_mode():
        for t in range(T):
            a = alg.act(d(g["obs_seq"][t]), d(g["priv_seq"][t]), d(g["hist_seq"][t]), eps=d(g["eps"][t]))
            np.testing.assert_allclose(a.cpu().numpy(), g["actions"][t], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(alg.transition.values.cpu().numpy(), g["values"][t], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(alg.transition.actions_log_prob.cpu().numpy(), g["logp"][t], rtol=1e-4,
                                       atol=2e-4)
            alg.process_env_step(d(g["rew"][t]), d(g["done"][t]).bool(), {})
        alg.compute_returns(d(g["obs_seq"][T]), d(g["priv_seq"][T]))
    np.testing.assert_allclose(alg.storage.returns.cpu().numpy(), g["returns"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(alg.storage.advantages.cpu().numpy(), g["advantages"], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(alg.storage.observations.cpu().numpy(), g["obs_seq"][:T])
    np.testing.assert_array_equal(alg.storage.privileged_observations.cpu().numpy(), g["priv_seq"][:T])
    np.testing.assert_array_equal(alg.storage.observation_histories.cpu().numpy(), g["hist_seq"][:T])
    assert not alg.storage.env_bins.any()
    alg.record_lr = True
    perm = torch.as_tensor(g["perm"], device=dev)
    orig = torch.randperm
    torch.randperm = lambda n, **kw: perm
    try:
        mv, ms, ma = alg.update()
    finally:
        torch.randperm = orig
    np.testing.assert_allclose(alg.lr_trace, g["lrs"], rtol=1e-9)
    assert ma == 0
    np.testing.assert_allclose([mv, ms], [g["mean_value_loss"], g["mean_surrogate_loss"]], rtol=2e-3, atol=1e-5)
    params = dict(ac.named_parameters())
    names = [str(x) for x in g["param_names"]]
    sums = np.array([params[k].detach().double().sum().item() for k in names])
    np.testing.assert_allclose(sums, g["param_sums"], rtol=2e-3, atol=2e-3)
    heads = np.stack([np.pad(params[k].detach().cpu().numpy().ravel()[:16], (0, max(0, 16 - params[k].numel())))
                      for k in names])
    np.testing.assert_allclose(heads, g["param_head"], rtol=2e-3, atol=1e-4)


# ---- 5. what a plain net refuses ------------------------------------------------------------------------------
def _last_error():
    msg = _abi.lib().lrl_last_error()
    return msg.decode() if msg else ""


def test_plain_net_refuses_adaptation_and_student_calls():
    """The adaptation phases and the student act need an adaptation module: on a plain net they return LRL_E_INVALID
    with a message and launch nothing (the output buffers keep their fill)."""
    n = 64
    ac = _hlp_ac()
    net = ac.flatten_parameters()
    L = _abi.lib()
    assert L.lrl_ppo_workspace_bytes(C.byref(net), C.c_int32(n)) > 0
    assert L.lrl_ppo_act_student_workspace_bytes(C.byref(net), C.c_int32(n)) < 0
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    grads = torch.full((net.total,), 3.0, device=dev)
    ctrl = torch.zeros(_abi.PPO_CTRL_BYTES // 8, dtype=torch.float64, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    rows = torch.arange(n, device=dev)
    batch = _abi.LrlPpoBatch()
    bufs = dict(obs=z(n, NO), priv=z(n, NP), hist=z(n, NH), actions=z(n, NA), values=z(n, 1), returns=z(n, 1),
                logp=z(n, 1), adv=z(n, 1), mu=z(n, NA), sigma=torch.ones(n, NA, device=dev))
    for k, t in bufs.items():
        setattr(batch, k, t.data_ptr())
    batch.rows, batch.batch, batch.hist_ld = rows.data_ptr(), n, NH
    rc = L.lrl_ppo_adaptation_forward_backward(C.byref(net), _p(ac._flat), None, _p(grads), C.byref(batch), _p(ws),
                                               _p(ctrl), _stream())
    assert rc == -1 and "plain" in _last_error()
    hp = _abi.LrlPpoHparams()
    m, v = torch.zeros_like(grads), torch.zeros_like(grads)
    before = ac._flat.clone()
    rc = L.lrl_ppo_adaptation_step(C.byref(net), _p(ac._flat), _p(grads), _p(m), _p(v), C.c_int64(1), C.c_double(1e-3),
                                   C.c_float(1.0), C.byref(hp), _p(ctrl), _stream())
    assert rc == -1 and "plain" in _last_error()
    mean = torch.full((n, NA), 5.0, device=dev)
    rc = L.lrl_ppo_act_student(C.byref(net), _p(ac._flat), _p(z(n, NO)), _p(z(n, NH)), C.c_int32(NH), C.c_int32(n),
                               _p(mean), None, _p(ws), _stream())
    assert rc == -1 and "plain" in _last_error()
    torch.cuda.synchronize()
    assert (grads == 3.0).all() and (mean == 5.0).all() and not ctrl.any() and not ws.any()
    assert torch.equal(ac._flat, before)
    with pytest.raises(RuntimeError):
        ac.act_student_fused(z(n, NO), z(n, NH))


def test_check_net_rejects_unsupported_combinations():
    """tanh is implemented for the plain form only: activation = 1 with plain = 0 (a tanh teacher / student net) is
    rejected by check_net, as are a plain ELU net, a plain net with an action count other than 3 / 12 or with encoder
    widths set, and field values outside {0, 1}.  The low-level descriptor (both fields zero) is still accepted."""
    import copy
    from lrl.ppo.actor_critic import ActorCritic
    L = _abi.lib()
    ok = lambda net: L.lrl_ppo_workspace_bytes(C.byref(net), C.c_int32(64)) > 0
    ll = ActorCritic(42, 18, 630, 12).cuda().flatten_parameters()
    assert (ll.activation, ll.plain) == (0, 0) and ok(ll)
    bad = copy.copy(ll)
    bad.activation = 1
    assert not ok(bad) and "plain" in _last_error()
    plain = _hlp_ac().flatten_parameters()
    assert ok(plain)
    for field, value in (("activation", 0), ("num_actions", 4), ("enc_h0", 256), ("latent", 18), ("ac_h2", 64),
                         ("plain", 2), ("activation", 2)):
        bad = copy.copy(plain)
        setattr(bad, field, value)
        assert not ok(bad), field
        assert _last_error()
    twelve = copy.copy(plain)
    twelve.num_actions = 12
    assert ok(twelve)


# ---- 6. one Runner.learn iteration over the navigation wrapper ------------------------------------------------
def test_runner_learn_one_iteration(tmp_path):
    from lrl.high_level import HighLevelControlWrapper
    from lrl.hlp import ActorCritic, Runner, RunnerArgs
    from lrl.ppo.actor_critic import ActorCritic as LowLevelActorCritic
    from lrl.ppo.runner import Logger
    ll = LowLevelActorCritic(42, 18, 630, 12)
    env = HighLevelControlWrapper.from_actor_critic(ll, num_envs=64, device=dev, robot="go1", seed=3)
    ll_before = {k: v.detach().clone() for k, v in ll.state_dict().items()}
    steps = RunnerArgs.num_steps_per_env
    RunnerArgs.num_steps_per_env = 8
    try:
        runner = Runner(env, device=dev, logger=Logger(str(tmp_path)))
    finally:
        RunnerArgs.num_steps_per_env = steps
    assert runner.num_steps_per_env == 8 and runner.alg.storage.num_envs == env.num_train_envs == 60
    ac = runner.alg.actor_critic
    assert isinstance(ac, ActorCritic) and runner.alg.fused
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    runner.alg.async_losses = False
    losses = []
    upd = runner.alg.update
    runner.alg.update = lambda: losses.append(upd()) or losses[-1]
    runner.learn(1, eval_freq=1, eval_expert=True)
    torch.cuda.synchronize()
    (mv, ms, ma), = losses
    assert np.isfinite([mv, ms]).all() and ma == 0
    after = ac.state_dict()
    assert len(after) == 17
    for k, v in after.items():
        assert torch.isfinite(v).all(), k
        if k.startswith(("actor_body", "critic_body")):
            assert not torch.equal(v, before[k]), k
    for k, v in ll.state_dict().items():  # the low-level policy under the wrapper is not trained
        assert torch.equal(v, ll_before[k]), k
    ck = os.path.join(str(tmp_path), "checkpoints")
    sd = torch.load(os.path.join(ck, "ac_weights_last.pt"), map_location="cpu", weights_only=True)
    with open(os.path.join(GOLDEN, "hlp_state_dict_keys.json")) as f:
        assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, list(s)) for k, s in json.load(f)]
    fresh = ActorCritic(NO, NP, NH, NA)
    fresh.load_state_dict(sd, strict=True)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, after[k].cpu()), k
    assert os.path.exists(os.path.join(ck, "ac_weights_000000.pt"))
    body = torch.jit.load(os.path.join(ck, "body_latest.jit"))
    x = torch.randn(5, NO)
    torch.testing.assert_close(body(x), fresh.actor_body(x))
    env.ll_env.env.close()
