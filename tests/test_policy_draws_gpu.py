"""The act kernels' policy noise (Box-Muller on the counter RNG's POLICY stream in act_fused_kernel and act_head_kernel
of csrc/lrl_ppo.hip) against tests/aux_ref.policy_normals: float64 arithmetic from the float32 uniforms of the Philox
restatement, a pair of actions sharing block j >> 1, u1 clamped at 1e-7f.

Each case calls act_fused with eps=None (the kernel draws) and again with eps = float32(policy_normals) (injected):
mu and the value must be equal bit for bit, and the drawn noise (a - mu) / sd must meet the reference within

    8 x 2^-24 rad + 4 x 2^-24 (|mu| / sd + |e_ref|)

(logf, sqrtf and sinf / cosf at 2 ulp each plus the product's rounding, relative to the radius; then the roundings of
mu + sd e and of the subtraction).  A wrong pair, word, stream or trig function moves e by O(1).  The log-prob is held
to float64 from the kernel's own a, mu, sd within 16 x 2^-24 sum_j (d^2 / (2 sd^2) + |ln sd| + ln sqrt(2 pi)).
tests/test_draws_ref.py shows on the CPU that a float32 numpy evaluation uses at most a quarter of the noise bar.

The three paths: LRL_ACT_FUSED=1 (act_fused_kernel), LRL_ACT_FUSED=0 (the GEMM chain's act_head_kernel), and the plain
tanh net of lrl.hlp (act_head_kernel at 3 actions: the last pair is half used).  Each case prints its largest ratio to
both bars.  Measured on an MI355X over every case (the float32 numpy evaluation on the CPU: 0.240 of the noise bar):

    path     largest |noise - reference| / bar    largest |lp - float64| / bar
    fused    0.278                                0.097
    chain    0.272                                0.114
    plain    0.253                                0.118
"""
import numpy as np
import pytest
import torch

import aux_ref as ar
import draws_cases as dc
from helpers import init_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
PATHS = ("fused", "chain", "plain")


def _net(path, no):
    """(ActorCritic with std = linspace(0.05, 1.5, NA), its RolloutStorage class, priv width, history width, NA)."""
    if path == "plain":
        from lrl.hlp import ActorCritic, RolloutStorage
        no, npriv, nh, na = 14, 18, 16, 3
    else:
        from lrl.ppo.actor_critic import ActorCritic
        from lrl.ppo.rollout_storage import RolloutStorage
        npriv, nh, na = 18, 15 * no, 12
    ac = ActorCritic(no, npriv, nh, na)
    init_params(ac)
    ac = ac.cuda()
    with torch.no_grad():  # ln sd changes sign over the actions, and a small sigma amplifies d
        ac.std.copy_(torch.linspace(0.05, 1.5, na))
    return ac, RolloutStorage, no, npriv, nh, na


def _act_twice(path, no, n, seed, counter, row_offset, monkeypatch, store=True):
    """The act with the kernel's own draws and with the reference normals injected, on the same inputs.  Returns the
    numpy results of both calls, the reference (e, rad), sd and the storage rows of the first call."""
    monkeypatch.setenv("LRL_ACT_FUSED", "1" if path == "fused" else "0")
    ac, Storage, no, npriv, nh, na = _net(path, no)
    g = torch.Generator(device=DEV).manual_seed(5)
    obs, priv, hist = (torch.randn(n, k, device=DEV, generator=g) for k in (no, npriv, nh))
    rows = row_offset + np.arange(n)
    e_ref, rad = ar.policy_normals_rows(rows, counter, seed, na)
    for i in {0, n // 2, n - 1}:  # the vectorised reference is the integer one
        e1, rad1 = ar.policy_normals(int(rows[i]), counter, seed, na)
        assert np.array_equal(e_ref[i], e1) and np.array_equal(rad[i], rad1)
    st = Storage(n, 3, [no], [npriv], [nh], [na], DEV) if store else None
    kw = dict(store=st.store_desc(), store_row=1) if store else {}
    drawn = ac.act_fused(obs, priv if path != "plain" or store else None, hist if store else None, seed=seed,
                         counter=counter, row_offset=row_offset, **kw)
    torch.cuda.synchronize()
    stored = None
    if store:
        stored = [x[1].detach().cpu().numpy().copy() for x in (st.actions, st.mu, st.sigma, st.values,
                                                                 st.actions_log_prob)]
        for t in (0, 2):
            assert not st.actions[t].any() and not st.values[t].any()
    drawn = [x.detach().cpu().numpy().copy() for x in drawn]
    eps = torch.as_tensor(e_ref.astype(F32), device=DEV).contiguous()
    injected = ac.act_fused(obs, priv if path != "plain" else None, eps=eps, seed=seed, counter=counter,
                            row_offset=row_offset)
    torch.cuda.synchronize()
    injected = [x.detach().cpu().numpy().copy() for x in injected]
    sd = ac.std.detach().cpu().numpy().copy()
    return drawn, injected, e_ref, rad, sd, stored


def _check(what, drawn, injected, e_ref, rad, sd, stored):
    a, mu, v, lp = drawn
    a2, mu2, v2, lp2 = injected
    n, na = a.shape
    assert all(np.isfinite(x).all() for x in drawn)
    assert np.array_equal(mu.view(np.uint32), mu2.view(np.uint32)), f"{what}: mu"
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)), f"{what}: value"
    a64, mu64, sd64 = a.astype(np.float64), mu.astype(np.float64), sd.astype(np.float64)[None, :]
    z = (a64 - mu64) / sd64
    bound = ar.policy_noise_bound(rad, e_ref, mu64 / sd64)
    ratio = np.abs(z - e_ref) / bound
    lp_terms, lp_mag = ar.log_prob_terms(a64, mu64, sd64)
    lp_bound = 16.0 * 2.0 ** -24 * lp_mag.sum(1)
    lp_ratio = np.abs(lp.astype(np.float64) - lp_terms.sum(1)) / lp_bound
    print(f"{what}: largest |noise - reference| / bar = {ratio.max():.3f}, largest |lp - float64| / bar = "
          f"{lp_ratio.max():.3f} (noise error {np.abs(z - e_ref).max():.3e}, lp error "
          f"{np.abs(lp - lp_terms.sum(1)).max():.3e})")
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (what, "noise", worst, z[worst], e_ref[worst], bound[worst])
    assert lp_ratio.max() <= 1.0, (what, "lp", int(np.argmax(lp_ratio)), lp_ratio.max())
    # the injected call samples mu + sd * float32(e_ref): the same actions within the same bar
    z2 = (a2.astype(np.float64) - mu64) / sd64
    assert (np.abs(z2 - e_ref) <= bound).all(), f"{what}: injected noise"
    if stored is not None:
        sa, sm, ss, sv, sl = stored
        for name, x, y in (("actions", sa, a), ("mu", sm, mu), ("values", sv.reshape(-1), v.reshape(-1)),
                           ("actions_log_prob", sl.reshape(-1), lp.reshape(-1)),
                           ("sigma", ss, np.broadcast_to(sd, (n, na)))):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), \
                f"{what}: stored {name}"
    return ratio, lp_ratio


@pytest.mark.parametrize("n,counter,row_offset", dc.ACT_CASES)
@pytest.mark.parametrize("path,no", [("fused", 42), ("fused", 235), ("chain", 42), ("chain", 235), ("plain", 14)])
def test_policy_noise_matches_philox_box_muller(path, no, n, counter, row_offset, monkeypatch):
    assert dc.ACT_SEED >> 32 != 0 and {c[0] for c in dc.ACT_CASES} == {1, 37, 300}
    res = _act_twice(path, no, n, dc.ACT_SEED, counter, row_offset, monkeypatch)
    _check(f"{path} no={no} n={n} counter={counter:#x} row_offset={row_offset}", *res)


@pytest.mark.parametrize("path", PATHS)
def test_the_clamped_uniform(path, monkeypatch):
    """Global row 2473292 (row 5 of 16) at seed 11, counter 3: u01 of block 1's first word is 0 exactly
    (test_draws_ref.py::test_the_clamped_key), so actions 2 and 3 take the radius of the clamp, sqrt(-2 ln 1e-7f)."""
    res = _act_twice(path, 42, 16, dc.CLAMP_SEED, dc.CLAMP_COUNTER, dc.CLAMP_ROW - 5, monkeypatch)
    ratio, lp_ratio = _check(f"{path} clamp", *res)
    (a, mu, v, lp), _, e_ref, rad, sd, _ = res
    na = a.shape[1]
    cols = [j for j in (2, 3) if j < na]  # (the plain net has 3 actions: action 2 alone)
    assert cols and all(rad[5, j] == np.sqrt(-2.0 * np.log(np.float64(F32(1e-7)))) for j in cols)
    assert np.isfinite(a[5, cols]).all() and np.isfinite(lp[5]) and (ratio[5, cols] <= 1.0).all()
    z = (a[5, cols].astype(np.float64) - mu[5, cols]) / sd[cols]
    assert np.abs(z).max() > 0.5  # (radius 5.68 at an angle of 0.223 turns: neither member is small)


@pytest.mark.parametrize("path", PATHS)
def test_pooled_statistics_per_action(path, monkeypatch):
    """8192 rows: per action (a - mu) / sd has its mean within 4 / sqrt(n) of 0 and its variance within 4 sqrt(2 / n)
    of 1 (the reference itself does: test_draws_ref.py), beside the per-draw bar."""
    n = dc.STATS_N
    res = _act_twice(path, 42, n, dc.ACT_SEED, dc.STATS_COUNTER, 0, monkeypatch, store=False)
    _check(f"{path} n={n}", *res)
    (a, mu, v, lp), _, e_ref, rad, sd, _ = res
    z = (a.astype(np.float64) - mu) / sd[None, :]
    se = 1.0 / np.sqrt(n)
    assert np.abs(z.mean(0)).max() <= 4 * se, z.mean(0)
    assert np.abs(z.var(0) - 1.0).max() <= 4 * np.sqrt(2.0) * se, z.var(0)
