"""The scalar arithmetic around the update's GEMMs, off its defaults and in isolation, through the C ABI:

A. the loss head (ppo_head_kernel, ELU and plain tanh form) at a non-unit std, non-unit old sigma and three
   hyper-parameter sets, against torch autograd of the reference's loss in float64 and fp32;
B. lrl_ppo_optimizer_step / lrl_ppo_adaptation_step on synthetic gradients against a float64 restatement of
   clip_grad_norm_ + Adam, the adaptive learning-rate table, the control block and what each call must leave alone;
C. lrl_gae / lrl_gae_partial / lrl_adv_normalize over ragged blocks, several waves and several blocks, against a
   float64 restatement of rollout_storage.py:76-90, and what they refuse.

Every input is drawn on the host from a seeded numpy generator, so the conditions on the inputs (clip fractions,
distance of every row from a branch of the loss) are properties of the float64 reference alone."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import autograd_minibatch, init_params
from lrl import _abi

pytestmark = pytest.mark.gpu
dev = "cuda:0"


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _last_error():
    msg = _abi.lib().lrl_last_error()
    return msg.decode() if msg else ""


def _hparams(**over):
    """The update's defaults (PPO_Args + torch.optim.Adam's) with fields overridden."""
    hp = _abi.LrlPpoHparams()
    _abi.fill(hp, clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=1.0, desired_kl=0.01,
              use_clipped_value_loss=1, adaptive_schedule=1, beta1=0.9, beta2=0.999, eps=1e-8)
    return _abi.fill(hp, **over)


def _make_ac(kind):
    """'teacher': the low-level ELU net ActorCritic(42, 18, 630, 12); 'plain': lrl.hlp's tanh net (14 obs, 3 actions).
    On the host, deterministic weights, std = linspace(0.3, 2.0, num_actions)."""
    if kind == "teacher":
        from lrl.ppo.actor_critic import ActorCritic
        ac = ActorCritic(42, 18, 630, 12)
    else:
        from lrl.hlp import ActorCritic
        ac = ActorCritic(14, 18, 16, 3)
    init_params(ac)
    with torch.no_grad():
        ac.std.copy_(torch.linspace(0.3, 2.0, ac.num_actions))
    return ac


# ---- A. the loss head away from unit std and the default hyper-parameters ---------------------------------------
HEAD_T, HEAD_N = 20, 37  # the storage: 37 envs x 20 steps
HP_SETS = {"narrow": dict(clip_param=0.1, entropy_coef=0.0, value_loss_coef=0.5, use_clipped_value_loss=1),
           "wide_unclipped": dict(clip_param=0.3, entropy_coef=0.05, value_loss_coef=2.0, use_clipped_value_loss=0),
           "defaults": dict(clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, use_clipped_value_loss=1)}
# a row closer than this to a branch of the loss (the ratio at 1 +- clip, V - values at +- clip, the two value losses
# equal) may take the other branch in fp32 — 1/batch of a gradient; fp32 log-probs of 12 actions carry ~1e-5
BRANCH_MARGIN = 1e-4


def head_inputs(ac, seed):
    """The storage of section A on the host (float32 tensors, [T * N, .]) for the host module ``ac``:
    old sigma = std * U(0.7, 1.3), old mu = mu_now + 0.2 std randn, actions = old mu + old sigma randn, old log-prob =
    the float64 log-prob of those actions under the current policy + 0.25 randn, values = V_now + 0.3 randn, returns =
    values + 0.3 randn, normalised randn advantages."""
    rng = np.random.default_rng(seed)
    R = HEAD_T * HEAD_N
    na = ac.num_actions
    nh = ac.adaptation_module[0].in_features if hasattr(ac, "adaptation_module") else ac.num_obs_history
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    obs, priv, hist = (f32(rng.standard_normal((R, k))) for k in (ac.num_obs, ac.num_privileged_obs, nh))
    m = copy.deepcopy(ac).double()
    with torch.no_grad():
        m.update_distribution(obs.double(), priv.double())
        mu_now = m.action_mean.numpy()
        v_now = m.evaluate(obs.double(), priv.double()).numpy()
        std = m.std.numpy()
    sigma = std * rng.uniform(0.7, 1.3, (R, na))
    mu = mu_now + 0.2 * std * rng.standard_normal((R, na))
    actions = f32(mu + sigma * rng.standard_normal((R, na)))
    a64 = actions.double().numpy()
    logp_now = (-(a64 - mu_now) ** 2 / (2 * std ** 2) - np.log(std) - 0.5 * np.log(2 * np.pi)).sum(-1, keepdims=True)
    logp = logp_now + 0.25 * rng.standard_normal((R, 1))
    values = v_now + 0.3 * rng.standard_normal((R, 1))
    returns = values + 0.3 * rng.standard_normal((R, 1))
    adv = rng.standard_normal((R, 1))
    adv = (adv - adv.mean()) / adv.std(ddof=1)
    return types.SimpleNamespace(obs=obs, priv=priv, hist=hist, actions=actions, values=f32(values),
                                 returns=f32(returns), logp=f32(logp), adv=f32(adv), mu=f32(mu), sigma=f32(sigma),
                                 rng=rng)


def head_rows(inp, batch):
    return torch.tensor(inp.rng.permutation(HEAD_T * HEAD_N)[:batch].astype(np.int64))


def head_reference(ac, inp, rows, args, dtype, teacher):
    b = tuple(t[rows] for t in (inp.obs, inp.actions, inp.values, inp.returns, inp.logp, inp.adv, inp.mu, inp.sigma))
    return autograd_minibatch(ac, args, b, dtype, priv=inp.priv[rows] if teacher else None,
                              hist=inp.hist[rows] if teacher else None), b


def head_input_conditions(r64, b, args):
    """On the float64 reference: both sides of the ratio clip (and of the value clip) hold at least 15 % of the rows,
    and no row sits within BRANCH_MARGIN of a branch.  Returns the fractions inside."""
    clip = args.clip_param
    ratio = r64.ratio.cpu().numpy()
    inside = np.abs(ratio - 1.0) <= clip
    frac = inside.mean()
    assert 0.15 <= frac <= 0.85, f"ratio inside the clip range: {frac:.2f}"
    assert np.abs(np.abs(ratio - 1.0) - clip).min() > BRANCH_MARGIN
    vfrac = None
    if args.use_clipped_value_loss:
        v = r64.value.cpu().numpy().ravel()
        tv, ret = b[2].double().cpu().numpy().ravel(), b[3].double().cpu().numpy().ravel()
        vin = np.abs(v - tv) <= clip
        vfrac = vin.mean()
        assert 0.15 <= vfrac <= 0.85, f"|V - values| inside the clip range: {vfrac:.2f}"
        assert np.abs(np.abs(v - tv) - clip).min() > BRANCH_MARGIN
        vc = tv + np.clip(v - tv, -clip, clip)
        assert np.abs((v - ret) ** 2 - (vc - ret) ** 2)[~vin].min() > BRANCH_MARGIN ** 2
    return frac, vfrac


# (net, minibatch rows, hyper-parameter set, seed): 185 rows = 5 full 32-row head workgroups + 25 rows; 7 rows: one
# partly filled workgroup.  The seeds are the first ones from 1 whose float64 reference meets head_input_conditions.
HEAD_CASES = [("teacher", 185, "narrow", 2), ("teacher", 185, "wide_unclipped", 1), ("teacher", 185, "defaults", 2),
              ("plain", 185, "narrow", 1), ("plain", 185, "wide_unclipped", 1), ("plain", 185, "defaults", 1),
              ("plain", 7, "defaults", 1)]


def _native_minibatch(ac, net, hp, inp, rows, teacher):
    """lrl_ppo_forward_backward (+ the adaptation call on the teacher net) on the device copies of ``inp``."""
    L = _abi.lib()
    mb = rows.numel()
    d = {k: getattr(inp, k).to(dev).contiguous() for k in ("obs", "priv", "hist", "actions", "values", "returns",
                                                            "logp", "adv", "mu", "sigma")}
    rows_d = rows.to(dev)
    nbytes = L.lrl_ppo_workspace_bytes(C.byref(net), C.c_int32(mb))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    grads = torch.full((net.total,), float("nan"), device=dev)
    ctrl = torch.zeros(_abi.PPO_CTRL_BYTES // 8, dtype=torch.float64, device=dev)
    batch = _abi.LrlPpoBatch()
    for k, t in d.items():
        setattr(batch, k, t.data_ptr())
    batch.rows, batch.batch, batch.hist_ld = rows_d.data_ptr(), mb, d["hist"].shape[1]
    _abi.check(L.lrl_ppo_forward_backward(C.byref(net), _p(ac._flat), _p(grads), C.byref(batch), C.byref(hp), _p(ws),
                                          _p(ctrl), _stream()))
    if teacher:
        _abi.check(L.lrl_ppo_adaptation_forward_backward(C.byref(net), _p(ac._flat), None, _p(grads), C.byref(batch),
                                                         _p(ws), _p(ctrl), _stream()))
    torch.cuda.synchronize()
    return grads, ctrl.view(torch.float32)[8:12].tolist()  # value, surrogate, adaptation, (kl in grads)


@pytest.mark.parametrize("kind,mb,hp_name,seed", HEAD_CASES)
def test_loss_head_off_unit_std_matches_autograd(kind, mb, hp_name, seed):
    """One minibatch of lrl_ppo_forward_backward with std = linspace(0.3, 2.0), old sigma = std * U(0.7, 1.3) and the
    hyper-parameter set, against torch autograd of the reference's loss: every gradient, the KL and the losses at the
    bars of test_native_minibatch_gradients_match_autograd (against fp32 autograd), and d loss / d std and the KL per
    component against float64 at 1e-4 |f64_j| + 1e-6 max_j |f64| — a bar fp32 autograd itself is first shown to meet.
    At std = 1 = old sigma, log std, 1/std against 1/std^2 and old sigma^2 in the KL are invisible."""
    teacher = kind == "teacher"
    args = types.SimpleNamespace(**HP_SETS[hp_name])
    ac = _make_ac(kind)
    inp = head_inputs(ac, seed)
    rows = head_rows(inp, mb)
    ac = ac.to(dev)
    net = ac.flatten_parameters()
    assert net.plain == (0 if teacher else 1)
    on = lambda x: types.SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(x).items()})
    inp_d, rows_d = on(inp), rows.to(dev)
    r64, b = head_reference(ac, inp_d, rows_d, args, torch.float64, teacher)
    r32, _ = head_reference(ac, inp_d, rows_d, args, torch.float32, teacher)
    frac, vfrac = head_input_conditions(r64, b, args)
    print(f"{kind} mb {mb} {hp_name}: ratio inside clip {frac:.2f}, value inside clip {vfrac}")
    grads, mbf = _native_minibatch(ac, net, _hparams(**HP_SETS[hp_name]), inp, rows, teacher)
    kl_native = grads[net.kl_slot].item()
    bad = []
    for name, prm in ac.named_parameters():
        off = (prm.data_ptr() - ac._flat.data_ptr()) // 4
        got = grads[off:off + prm.numel()].view_as(prm)
        ref, ref64 = r32.grads[name], r64.grads[name]
        if ref is None:  # (no gradient reaches it: not the case for either net)
            bad.append(f"{name}: no reference gradient")
            continue
        err = (got - ref).abs().max().item()
        e_nat, e_t32 = (got.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
        print(f"  {name}: |native - fp32| {err:.3e} (ref max {ref.abs().max().item():.3e}); vs float64: native "
              f"{e_nat:.3e} torch-fp32 {e_t32:.3e}")
        if not err <= 1e-4 * (ref.abs().max().item() + 1e-6) + 1e-7:
            bad.append(f"{name}: err {err:.3g} ref max {ref.abs().max().item():.3g} got max {got.abs().max().item():.3g}")
    print(f"  kl {kl_native:.8e} / fp32 {r32.kl:.8e} / f64 {r64.kl:.8e}; value {mbf[0]:.8e} / {r32.value_loss:.8e}; "
          f"surrogate {mbf[1]:.8e} / {r32.surrogate:.8e}")
    np.testing.assert_allclose(kl_native, r32.kl, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(mbf[:2], [r32.value_loss, r32.surrogate], rtol=1e-4, atol=1e-7)
    if teacher:
        np.testing.assert_allclose(mbf[2], r32.adaptation_loss, rtol=1e-4, atol=1e-7)
    assert not bad, "\n".join(bad)
    # d loss / d std and the KL against float64, per component
    s64 = r64.grads["std"].cpu().numpy()
    bar = 1e-4 * np.abs(s64) + 1e-6 * np.abs(s64).max()
    s32 = r32.grads["std"].double().cpu().numpy()
    snat = grads[net.std_off:net.std_off + ac.num_actions].double().cpu().numpy()
    kl_bar = (1e-4 + 1e-6) * abs(r64.kl)
    print(f"  d/d std vs float64, worst error / bar: native {(np.abs(snat - s64) / bar).max():.3f} torch-fp32 "
          f"{(np.abs(s32 - s64) / bar).max():.3f}; kl: native {abs(kl_native - r64.kl) / kl_bar:.3f} torch-fp32 "
          f"{abs(r32.kl - r64.kl) / kl_bar:.3f}")
    assert (np.abs(s32 - s64) <= bar).all() and abs(r32.kl - r64.kl) <= kl_bar, "fp32 autograd misses the bar: inputs"
    assert (np.abs(snat - s64) <= bar).all(), (snat, s64)
    assert abs(kl_native - r64.kl) <= kl_bar


# ---- B. the optimiser step in isolation --------------------------------------------------------------------------
def adam_reference(p, g, m, v, step, lr, scale, hp, clip=True):
    """clip_grad_norm_(max_grad_norm) + one torch.optim.Adam step, float64, over whole arrays: g = grads * scale,
    clip = min(max_norm / (|g| + 1e-6), 1), step `step` with lr / bc1 and sqrt(v) / sqrt(bc2) + eps.  Returns
    (p, m, v, total_norm, clip)."""
    b1, b2, eps = float(hp.beta1), float(hp.beta2), float(hp.eps)
    g = np.asarray(g, np.float64) * scale
    norm = float(np.sqrt(np.sum(g * g)))
    c = min(float(hp.max_grad_norm) / (norm + 1e-6), 1.0) if clip else 1.0
    g = g * c
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v, norm, c


def next_lr(lr, kl, hp):
    """ppo.py:113-124 in Python doubles, on the kl the device forms (an fp32 product) and the fp32 desired_kl."""
    if hp.adaptive_schedule:
        if kl > float(hp.desired_kl) * 2.0:
            return max(1e-5, lr / 1.5)
        if float(hp.desired_kl) / 2.0 > kl > 0.0:
            return min(1e-2, lr * 1.5)
    return lr


def log_uniform_grads(rng, sign, norm):
    """Magnitudes log-uniform over 1e-7 .. 1e-1 (so eps = 1e-8 matters in Adam's denominator) with the given signs,
    rescaled to the 2-norm ``norm``; float32."""
    g = sign * 10.0 ** rng.uniform(-7.0, -1.0, sign.shape)
    return (g * (norm / np.sqrt(np.sum(g * g)))).astype(np.float32)


def test_adam_reference_matches_torch():
    """The float64 restatement against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64 (host only):
    three steps, a clipped and an unclipped norm, grad_scale 1 and 0.5."""
    hp = _hparams()
    rng = np.random.default_rng(0)
    n = 1000
    sign = rng.choice([-1.0, 1.0], n)
    for norm, scale in ((0.5, 1.0), (4.0, 1.0), (4.0, 0.5)):
        p0 = rng.standard_normal(n)
        pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([pt], lr=1e-3, betas=(float(hp.beta1), float(hp.beta2)), eps=float(hp.eps))
        p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
        for step in (1, 2, 3):
            g = log_uniform_grads(rng, sign, norm)
            pt.grad = torch.tensor(g, dtype=torch.float64) * scale
            tn = torch.nn.utils.clip_grad_norm_([pt], float(hp.max_grad_norm)).item()
            opt.step()
            p, m, v, tot, c = adam_reference(p, g, m, v, step, 1e-3, scale, hp)
            assert (c < 1.0) == (norm * scale > 1.0)
            np.testing.assert_allclose(tot, tn, rtol=1e-13)
            st = opt.state[pt]
            np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12)


def _descriptor(which):
    """(net, mask of the flat buffer's parameter elements).  'teacher': main range ~0.45 M floats (the grid-stride
    path); 'plain': the navigation net; 'plain_heads': the plain net's descriptor with the main range narrowed to its
    heads and std (643 floats from a non-zero main_begin: 253 of the 256 norm blocks see no element)."""
    ac = _make_ac("teacher" if which == "teacher" else "plain").to(dev)
    net = ac.flatten_parameters()
    mask = np.zeros(net.total, bool)
    for prm in ac.parameters():
        off = (prm.data_ptr() - ac._flat.data_ptr()) // 4
        mask[off:off + prm.numel()] = True
    if which == "plain_heads":
        net = copy.copy(net)
        net.main_begin = net.w4a
        assert 0 < net.main_end - net.main_begin < 1024
    return net, mask


def _ctrl_dev(lr, loss_sum, mb):
    c = np.zeros(1, dtype=[("lr", "f8"), ("loss_sum", "f8", 3), ("mb", "f4", 4), ("clip_scale", "f4"),
                           ("step_size", "f4"), ("total_norm", "f4"), ("pad", "f4")])
    assert c.itemsize == _abi.PPO_CTRL_BYTES
    c["lr"], c["loss_sum"], c["mb"] = lr, loss_sum, mb
    c["clip_scale"], c["step_size"], c["total_norm"], c["pad"] = -1.0, -2.0, -3.0, -4.0
    return torch.tensor(c.view(np.uint8), device=dev), c.dtype


def _ctrl_host(t, dt):
    return t.cpu().numpy().view(dt)[0]


SENT_P, SENT_M, SENT_V, SENT_G = 7.0, -3.0, 5.0, 1e6  # outside the range a step owns


class _OptState:
    """Synthetic flat buffers for a descriptor: parameters, moments (zero, or random with v >= 0) inside the region
    [lo, hi) at the parameter positions, zero in its alignment gaps, sentinels everywhere else."""

    def __init__(self, net, mask, lo, hi, seed, random_moments):
        self.net, self.lo, self.hi = net, lo, hi
        self.rng = rng = np.random.default_rng(seed)
        n = net.total
        self.own = np.zeros(n, bool)
        self.own[lo:hi] = True
        self.live = self.own & mask  # the region's parameter elements; own & ~mask: its alignment gaps
        k = int(self.live.sum())
        # one sign per element for gradients and first moments: no cancellation in m + (1 - b1)(g - m), so the
        # relative bar on the moments measures the kernel's rounding alone
        self.sign = rng.choice([-1.0, 1.0], k)
        p = np.full(n, SENT_P, np.float32)
        m = np.full(n, SENT_M, np.float32)
        v = np.full(n, SENT_V, np.float32)
        p[self.own], m[self.own], v[self.own] = 0.0, 0.0, 0.0
        p[self.live] = (0.1 * rng.standard_normal(k)).astype(np.float32)
        if random_moments:  # |m| / sqrt(v) <= 1 as in a real Adam state, so the update stays a fraction of lr
            m0 = (self.sign * 10.0 ** rng.uniform(-6.0, -2.0, k)).astype(np.float32)
            m[self.live] = m0
            v[self.live] = ((m0.astype(np.float64) * rng.uniform(1.0, 3.0, k)) ** 2).astype(np.float32)
        self.p, self.m, self.v = (torch.tensor(a, device=dev) for a in (p, m, v))
        self.p64, self.m64, self.v64 = (a[self.live].astype(np.float64) for a in (p, m, v))
        self.before = [t.clone() for t in (self.p, self.m, self.v)]

    def grads(self, norm, kl_slot_value):
        """A fresh gradient buffer: log-uniform magnitudes of 2-norm ``norm`` at the region's parameters, zero in its
        gaps, 1e6 everywhere else (the other region included), the KL in its slot."""
        g = np.full(self.net.total, SENT_G, np.float32)
        g[self.own] = 0.0
        g[self.live] = log_uniform_grads(self.rng, self.sign, norm)
        g[self.net.kl_slot] = kl_slot_value
        return g

    def check_isolation(self, g_dev, g_host):
        """Everything outside [lo, hi) is bit-identical (the gradient buffer everywhere); the region's alignment gaps
        are still exactly zero."""
        assert torch.equal(g_dev.cpu(), torch.tensor(g_host))
        out = torch.tensor(~self.own, device=dev)
        gap = torch.tensor(self.own & ~self.live, device=dev)
        for t, t0 in zip((self.p, self.m, self.v), self.before):
            assert torch.equal(t[out], t0[out])
            assert torch.isfinite(t[gap]).all() and (t[gap] == 0).all()


def _compare_state(s, n_steps, lr_used, worst):
    """Moments at rtol 1e-6 (+ 1e-30 for zeros); parameters after n steps within n (2^-23 |p| + 1e-5 lr): one rounding
    of p per step, plus ~10 fp32 roundings of an update bounded by a few lr.  Records the worst error / bar."""
    live = torch.tensor(s.live, device=dev)
    p, m, v = (t[live].double().cpu().numpy() for t in (s.p, s.m, s.v))
    for name, got, ref in (("exp_avg", m, s.m64), ("exp_avg_sq", v, s.v64)):
        r = (np.abs(got - ref) / (1e-6 * np.abs(ref) + 1e-30)).max()
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, (name, r)
    bar = n_steps * (2.0 ** -23 * np.abs(s.p64) + 1e-5 * lr_used)
    r = (np.abs(p - s.p64) / bar).max()
    worst["params"] = max(worst.get("params", 0.0), r)
    assert r <= 1.0, ("params", r)


OPT_CASES = [  # (descriptor, gradient norm, grad_scale, steps, random moments)
    ("teacher", 0.5, 1.0, (1, 2, 3), False), ("teacher", 4.0, 1.0, (1, 2, 3), False),
    ("teacher", 4.0, 0.5, (1, 2, 3), False), ("teacher", 1.6, 0.5, (57,), True), ("teacher", 4.0, 1.0, (57,), True),
    ("plain", 0.5, 1.0, (1, 2, 3), False), ("plain", 4.0, 0.5, (1, 2, 3), False), ("plain", 1.6, 0.5, (57,), True),
    ("plain_heads", 0.5, 0.5, (1, 2, 3), False), ("plain_heads", 4.0, 1.0, (1, 2, 3), False),
    ("plain_heads", 4.0, 1.0, (57,), True)]


@pytest.mark.parametrize("which,norm,scale,steps,random_moments", OPT_CASES)
def test_optimizer_step_matches_float64(which, norm, scale, steps, random_moments):
    """lrl_ppo_optimizer_step (sum of squares -> finalize -> Adam) on synthetic buffers against adam_reference started
    from the same fp32 values, max_grad_norm = 1: the norm of the scaled gradients below it (0.5, 1.6 x 0.5: no clip) and
    above (4.0, 4.0 x 0.5), steps 1, 2, 3 from zero moments or step 57 from random ones.  The control block after each
    call, and bit-identity of everything outside [main_begin, main_end) — the adaptation region's gradients are 1e6
    and must not reach the norm."""
    L = _abi.lib()
    net, mask = _descriptor(which)
    hp = _hparams(adaptive_schedule=0)
    s = _OptState(net, mask, net.main_begin, net.main_end, seed=len(which) + int(10 * norm) + steps[0],
                  random_moments=random_moments)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    lr = 1e-3
    mb = [0.125, -0.375, 0.3, 9.0]
    loss_sum = [1.25, -0.5, 3.0]
    ctrl, dt = _ctrl_dev(lr, loss_sum, mb)
    worst = {}
    kl = 0.03
    for n_done, step in enumerate(steps, 1):
        g = s.grads(norm, kl)
        g_dev = torch.tensor(g, device=dev)
        _abi.check(L.lrl_ppo_optimizer_step(C.byref(net), _p(s.p), _p(g_dev), _p(s.m), _p(s.v), C.c_int64(step),
                                            C.c_float(scale), C.byref(hp), _p(ws), _p(ctrl), _stream()))
        torch.cuda.synchronize()
        s.p64, s.m64, s.v64, tot, clip = adam_reference(s.p64, g[s.live], s.m64, s.v64, step, lr, scale, hp)
        assert (clip < 1.0) == (norm * scale > 1.0)
        c = _ctrl_host(ctrl, dt)
        assert c["lr"] == lr  # adaptive_schedule = 0: whatever the KL
        assert c["mb"][3] == np.float32(kl) * np.float32(scale)
        np.testing.assert_allclose(c["total_norm"], tot, rtol=1e-6)
        np.testing.assert_allclose(c["clip_scale"], clip, rtol=1e-6)
        assert c["step_size"] == np.float32(lr / (1.0 - float(hp.beta1) ** step))
        for k in (0, 1):
            loss_sum[k] += float(np.float32(mb[k]))
        assert list(c["loss_sum"]) == loss_sum and list(c["mb"][:3]) == [np.float32(x) for x in mb[:3]]
        assert c["pad"] == -4.0
        s.check_isolation(g_dev, g)
        _compare_state(s, n_done, lr, worst)
    print(f"optimizer_step {which} norm {norm} scale {scale} steps {steps}: worst error / bar "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


LR_TABLE = [  # (lr, KL slot, grad_scale, adaptive) -> expected through next_lr
    (1e-3, 0.03, 1.0, 1), (1e-3, 0.0201, 1.0, 1), (1e-3, 0.0199, 1.0, 1), (1e-3, 0.0051, 1.0, 1),
    (1e-3, 0.0049, 1.0, 1), (1e-3, 1e-12, 1.0, 1), (1e-3, 0.0, 1.0, 1), (1e-3, -1e-3, 1.0, 1),
    (1.2e-5, 0.03, 1.0, 1), (8e-3, 0.0049, 1.0, 1), (1e-3, 0.03, 1.0, 0), (1e-3, 0.0049, 1.0, 0), (1e-3, 0.0, 1.0, 0),
    (1e-3, 0.0402, 0.5, 1), (1e-3, 0.0098, 0.5, 1), (1e-3, 0.0398, 0.5, 1)]
LR_EXPECT = ["down", "down", "same", "same", "up", "up", "same", "same", 1e-5, 1e-2, "same", "same", "same", "down", "up",
             "same"]


def test_adaptive_learning_rate_table():
    """The device-side schedule (ppo.py:113-124) at desired_kl = 0.01, exactly: above 2 x desired the rate is divided
    by 1.5, below half of it (and above zero) multiplied, with the 1e-5 / 1e-2 caps, the k > 0 guard, no change under
    adaptive_schedule = 0, and grad_scale applied to the KL before the comparison.  Equality is exact: the same
    expression in Python doubles."""
    L = _abi.lib()
    net, mask = _descriptor("plain_heads")
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for (lr, kl, scale, adaptive), want in zip(LR_TABLE, LR_EXPECT):
        hp = _hparams(adaptive_schedule=adaptive)
        s = _OptState(net, mask, net.main_begin, net.main_end, seed=3, random_moments=False)
        g = s.grads(0.5, kl)
        g_dev = torch.tensor(g, device=dev)
        ctrl, dt = _ctrl_dev(lr, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])
        _abi.check(L.lrl_ppo_optimizer_step(C.byref(net), _p(s.p), _p(g_dev), _p(s.m), _p(s.v), C.c_int64(1),
                                            C.c_float(scale), C.byref(hp), _p(ws), _p(ctrl), _stream()))
        torch.cuda.synchronize()
        c = _ctrl_host(ctrl, dt)
        k = float(np.float32(kl) * np.float32(scale))
        expect = next_lr(lr, k, hp)
        table = {"down": max(1e-5, lr / 1.5), "up": min(1e-2, lr * 1.5), "same": lr}.get(want, want)
        assert expect == table, (lr, kl, scale, adaptive)  # the restatement agrees with the table
        assert c["lr"] == expect, (lr, kl, scale, adaptive, c["lr"])
        assert c["mb"][3] == np.float32(kl) * np.float32(scale)
        assert c["step_size"] == np.float32(expect / (1.0 - float(hp.beta1)))
        s.check_isolation(g_dev, g)  # (the KL slot is read, never written)


@pytest.mark.parametrize("norm,scale,steps,random_moments,with_ctrl",
                         [(0.5, 1.0, (1, 2, 3), False, True), (4.0, 0.5, (1, 2, 3), False, True),
                          (4.0, 1.0, (57,), True, False)])
def test_adaptation_step_matches_float64(norm, scale, steps, random_moments, with_ctrl):
    """lrl_ppo_adaptation_step, the mirror image: Adam at the host's learning rate over [adapt_begin, adapt_end) alone,
    grad_scale applied, no clip (a norm of 4 passes unclipped), loss_sum[2] += mb[2] and nothing else of the control
    block — and the same step with ctrl = NULL."""
    L = _abi.lib()
    net, mask = _descriptor("teacher")
    hp = _hparams()
    s = _OptState(net, mask, net.adapt_begin, net.adapt_end, seed=int(10 * norm) + steps[0], random_moments=random_moments)
    lr = 2.5e-3
    mb = [0.125, -0.375, 0.3, 9.0]
    loss_sum = [1.25, -0.5, 3.0]
    ctrl, dt = _ctrl_dev(7e-4, loss_sum, mb)
    c0 = _ctrl_host(ctrl, dt).copy()
    worst = {}
    for n_done, step in enumerate(steps, 1):
        g = s.grads(norm, 0.03)
        g_dev = torch.tensor(g, device=dev)
        _abi.check(L.lrl_ppo_adaptation_step(C.byref(net), _p(s.p), _p(g_dev), _p(s.m), _p(s.v), C.c_int64(step),
                                             C.c_double(lr), C.c_float(scale), C.byref(hp),
                                             _p(ctrl) if with_ctrl else None, _stream()))
        torch.cuda.synchronize()
        s.p64, s.m64, s.v64, _, clip = adam_reference(s.p64, g[s.live], s.m64, s.v64, step, lr, scale, hp, clip=False)
        c = _ctrl_host(ctrl, dt)
        if with_ctrl:
            loss_sum[2] += float(np.float32(mb[2]))
        assert list(c["loss_sum"]) == loss_sum
        for k in ("lr", "clip_scale", "step_size", "total_norm", "pad"):
            assert c[k] == c0[k], k
        assert list(c["mb"]) == list(c0["mb"])
        s.check_isolation(g_dev, g)
        _compare_state(s, n_done, lr, worst)
    print(f"adaptation_step norm {norm} scale {scale} steps {steps}: worst error / bar "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- C. GAE over more than one wave and block --------------------------------------------------------------------
GAMMA, LAM = 0.99, 0.95


def gae_reference(rew, done, val, last, gamma=GAMMA, lam=LAM):
    """rollout_storage.py:76-90 in float64: (returns, raw advantages)."""
    rew, val, last = (np.asarray(a, np.float64) for a in (rew, val, last))
    T = rew.shape[0]
    ret = np.empty_like(rew)
    adv = 0.0
    for t in reversed(range(T)):
        nv = last if t == T - 1 else val[t + 1]
        nt = 1.0 - done[t].astype(np.float64)
        delta = rew[t] + nt * gamma * nv - val[t]
        adv = delta + nt * gamma * lam * adv
        ret[t] = adv + val[t]
    return ret, ret - val


def normalize_reference(adv, stats):
    """(adv - mean) / (unbiased std + 1e-8) from stats = (sum, sum of squares, count), float64."""
    s1, s2, n = stats
    mean = s1 / n
    var = (s2 - n * mean * mean) / (n - 1.0)
    return (np.asarray(adv, np.float64) - mean) / (np.sqrt(max(var, 0.0)) + 1e-8)


def gae_inputs(T, N, shift, seed):
    """Dones at ~10 %, one env done at every step and one never (N >= 2); rewards = randn + shift."""
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((T, N)) + shift).astype(np.float32)
    val = rng.standard_normal((T, N)).astype(np.float32)
    last = rng.standard_normal(N).astype(np.float32)
    done = (rng.random((T, N)) < 0.1).astype(np.uint8)
    if N >= 2:
        done[:, 0], done[:, N - 1] = 1, 0
    return rew, done, val, last


def _stats64(a):
    a = np.asarray(a, np.float64).ravel()
    return np.array([a.sum(), (a * a).sum(), float(a.size)])


# one lane; a ragged wave; one lane of a second wave; one lane of a second block; four blocks, the last ragged; T = 1
# over two blocks.  shift = 5 moves the advantage mean away from zero: by 1.6 standard deviations at lam = 0.95 (the
# advantages then grow with the steps left to the horizon, which spreads them), by 3.8 at lam = 0.5.
GAE_CASES = [(24, 1, 0.0, GAMMA, LAM), (24, 63, 0.0, GAMMA, LAM), (24, 65, 0.0, GAMMA, LAM), (24, 257, 0.0, GAMMA, LAM),
             (24, 1000, 0.0, GAMMA, LAM), (1, 300, 0.0, GAMMA, LAM), (24, 257, 5.0, GAMMA, LAM), (24, 257, 5.0, GAMMA, 0.5)]


def _gae_call(name, bufs, T, N, gamma, lam, ret, adv, ws, stats=None):
    L = _abi.lib()
    args = [_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), C.c_int32(T), C.c_int32(N), C.c_float(gamma),
            C.c_float(lam), _p(ret), _p(adv), _p(ws)]
    if name == "lrl_gae_partial":
        args.append(_p(stats))
    rc = getattr(L, name)(*args, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("T,N,shift,gamma,lam", GAE_CASES)
def test_gae_shapes_against_float64(T, N, shift, gamma, lam):
    """lrl_gae_partial: returns / raw advantages at the bars of test_gae_matches_reference, stats = (sum, sum of
    squares, T * N) of the fp32 advantages it wrote; lrl_adv_normalize with the stats of this shard and a second one;
    lrl_gae bit-identical to the two calls with the shard's own stats, and within 1e-5 of the float64 normalisation."""
    L = _abi.lib()
    rew, done, val, last = gae_inputs(T, N, shift, seed=T * 1000 + N)
    ret64, adv64 = gae_reference(rew, done, val, last, gamma, lam)
    if shift:
        ratio = abs(adv64.mean()) / adv64.std(ddof=1)
        print(f"gae {T}x{N} shift {shift}: |mean| / std of the raw advantages {ratio:.2f}")
        assert ratio > (3.0 if lam == 0.5 else 1.5)
    bufs = [torch.tensor(a, device=dev) for a in (rew, done, val, last)]
    new = lambda: torch.full((T, N), float("nan"), device=dev)
    ws = torch.zeros(4096, device=dev)
    ret, adv, stats = new(), new(), torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    _abi.check(_gae_call("lrl_gae_partial", bufs, T, N, gamma, lam, ret, adv, ws, stats))
    raw = adv.cpu().numpy()
    np.testing.assert_allclose(ret.cpu().numpy(), ret64, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(raw, adv64, rtol=1e-5, atol=1e-5)
    own = _stats64(raw)
    np.testing.assert_allclose(stats.cpu().numpy(), own, rtol=1e-10, atol=0)
    # the multi-GPU split: stats of this shard and another one, as the all-reduce delivers them
    other = (np.random.default_rng(N).standard_normal(3 * T * N + 5) * 1.7 + 0.4 + shift).astype(np.float32)
    both = own + _stats64(other)
    adv2 = adv.clone()
    both_d = torch.tensor(both, device=dev)
    _abi.check(L.lrl_adv_normalize(_p(adv2), C.c_int64(T * N), _p(both_d), _stream()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(adv2.cpu().numpy(), normalize_reference(raw, both), rtol=1e-5, atol=1e-5)
    assert torch.equal(both_d.cpu(), torch.tensor(both)) and torch.equal(adv.cpu(), torch.tensor(raw))
    # lrl_gae = partial + normalize with the shard's own stats, bit for bit
    adv3 = adv.clone()
    _abi.check(L.lrl_adv_normalize(_p(adv3), C.c_int64(T * N), _p(stats), _stream()))
    ret1, adv1, ws1 = new(), new(), torch.zeros(4096, device=dev)
    _abi.check(_gae_call("lrl_gae", bufs, T, N, gamma, lam, ret1, adv1, ws1))
    assert torch.equal(ret1, ret) and torch.equal(adv1, adv3)
    np.testing.assert_allclose(adv1.cpu().numpy(), normalize_reference(raw, own), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(adv1.cpu().numpy(), normalize_reference(adv64, _stats64(adv64)), rtol=1e-5, atol=1e-5)


def test_gae_refusals_launch_nothing():
    """N = 256001 (more partials than the workspace holds), T = 0 and a null pointer: non-zero with a message, and the
    sentinel-filled outputs untouched (nothing is launched, so tiny buffers serve)."""
    L = _abi.lib()
    n = 8
    bufs = [torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, device=dev),
            torch.zeros(n, device=dev)]
    ret, adv = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    ws = torch.full((4096,), 7.0, device=dev)
    stats = torch.full((3,), 7.0, dtype=torch.float64, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return all((t == 7.0).all().item() for t in (ret, adv, ws, stats))

    for name in ("lrl_gae", "lrl_gae_partial"):
        for T, N in ((1, 256001), (0, 8), (1, 0)):
            assert _gae_call(name, bufs, T, N, GAMMA, LAM, ret, adv, ws, stats) != 0
            assert "lrl_gae" in _last_error() and untouched(), (name, T, N)
        for k in range(4):
            nb = list(bufs)
            nb[k] = None
            assert _gae_call(name, nb, 1, n, GAMMA, LAM, ret, adv, ws, stats) != 0
            assert "lrl_gae" in _last_error() and untouched(), (name, k)
        for r, a, w in ((None, adv, ws), (ret, None, ws), (ret, adv, None)):
            assert _gae_call(name, bufs, 1, n, GAMMA, LAM, r, a, w, stats) != 0
            assert "lrl_gae" in _last_error() and untouched(), name
    assert _gae_call("lrl_gae_partial", bufs, 1, n, GAMMA, LAM, ret, adv, ws, None) != 0 and untouched()
    for a, total, s in ((None, 8, stats), (adv, 8, None), (adv, 1, stats), (adv, 0, stats)):
        assert L.lrl_adv_normalize(_p(a), C.c_int64(total), _p(s), _stream()) != 0
        assert "lrl_adv_normalize" in _last_error() and untouched()
