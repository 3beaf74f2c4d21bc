"""The one-launch rollout act (act_fused_kernel's whole-act instance: x6 bodies on LDS plane images, one workgroup per
32-row tile and group) against the GEMM-chain act (LRL_ACT_FUSED=0: the encoder launch, three gemm_x6_kernel products
and act_head_kernel) on the same inputs: every output and every array of the storage row bit for bit (torch.equal).

The kernel's body products take the chain's x6 steps (x6_mma over 16-k steps from k = 0), which the chain itself only
takes from 64 rows on (gemm_x6_kernel's smallest batch; below it the chain's products run on the fp32 MFMA, whose
roundings an x6 product cannot reproduce).  So under 64 rows every setting of LRL_ACT_FUSED runs the chain, and the
cases n = 1, 31, 32, 33 compare the chain with itself; the same remainders — a lone row, 31, a whole tile, a tile and
one row — are also run behind whole tiles (n = 65, 95, 64 / 160, 97), where LRL_ACT_FUSED=1 is the one-launch act.

Before each call the outputs and the whole rollout storage are NaN: a row or field the kernel skips shows as NaN in
the storage row, and a write outside the storage row shows as a number in another row.
"""
import ctypes as C

import pytest
import torch

from helpers import init_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NA = 12
NS = (1, 31, 32, 33, 95, 160, 64, 65, 97, 127)
T = 3  # storage rows
FIELDS = ("observations", "privileged_observations", "observation_histories", "actions", "mu", "sigma", "values",
          "actions_log_prob")

_nets = {}


def _net(no):
    """The ActorCritic over `no` observations (42: the presets' net; 235: the perceptive one, X pitch 256), built once."""
    if no not in _nets:
        from lrl.ppo.actor_critic import ActorCritic
        ac = ActorCritic(no, 18, 15 * no, NA)
        init_params(ac)
        ac = ac.cuda()
        with torch.no_grad():
            ac.std.copy_(torch.linspace(0.5, 1.5, NA))
        _nets[no] = ac
    return _nets[no]


def _inputs(n, no, seed=7):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return tuple(torch.randn(n, k, device=DEV, generator=g) for k in (no, 18, 15 * no, NA))


def _act(ac, obs, priv, hist, eps, row_offset, st, store_row, want=("actions", "mu", "values", "logp")):
    """lrl_ppo_act on NaN-filled outputs (and a NaN-filled storage `st`, or None).  Returns the requested outputs."""
    from lrl import _abi
    n = obs.shape[0]
    net = ac.flatten_parameters()
    L = _abi.lib()
    nbytes = L.lrl_ppo_act_workspace_bytes(C.byref(net), n)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    out = {"actions": torch.full((n, NA), float("nan"), device=DEV), "mu": torch.full((n, NA), float("nan"), device=DEV),
           "values": torch.full((n, 1), float("nan"), device=DEV), "logp": torch.full((n,), float("nan"), device=DEV)}
    if st is not None:
        for f in FIELDS:
            getattr(st, f).fill_(float("nan"))
    ptr = {k: (v.data_ptr() if k in want else None) for k, v in out.items()}
    _abi.check(L.lrl_ppo_act(net, ac._flat.data_ptr(), obs.data_ptr(), priv.data_ptr(), hist.data_ptr(), n,
                             eps.data_ptr() if eps is not None else None, 11, 3, row_offset, ptr["actions"], ptr["mu"],
                             ptr["values"], ptr["logp"], st.store_desc() if st is not None else None, store_row,
                             ws.data_ptr(), _abi.stream_of(torch.device(DEV))))
    torch.cuda.synchronize()
    return out


def _both(monkeypatch, call):
    """call() under LRL_ACT_FUSED=1 and =0."""
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LRL_ACT_FUSED", fused)
        res.append(call())
    return res


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("no", [42, 235])
def test_one_launch_act_equals_chain_bit_for_bit(no, n, monkeypatch):
    from lrl.ppo.rollout_storage import RolloutStorage
    ac = _net(no)
    obs, priv, hist, eps = _inputs(n, no)
    st = RolloutStorage(n, T, [no], [18], [15 * no], [NA], DEV)
    for inject in (True, False):
        for row_offset in (0, 64):
            for store_row in (0, T - 1):
                what = f"no={no} n={n} inject={inject} row_offset={row_offset} store_row={store_row}"

                def call():
                    out = _act(ac, obs, priv, hist, eps if inject else None, row_offset, st, store_row)
                    return out, {f: getattr(st, f).clone() for f in FIELDS}
                (o1, s1), (o0, s0) = _both(monkeypatch, call)
                for k in o1:
                    assert not torch.isnan(o1[k]).any() and not torch.isnan(o0[k]).any(), f"{what}: {k} has skipped rows"
                    assert torch.equal(o1[k], o0[k]), f"{what}: {k}"
                for f in FIELDS:
                    a, b = s1[f], s0[f]
                    assert not torch.isnan(a[store_row]).any() and not torch.isnan(b[store_row]).any(), \
                        f"{what}: storage {f} has skipped rows"
                    assert torch.equal(a[store_row], b[store_row]), f"{what}: storage {f}"
                    for t in range(T):
                        if t != store_row:
                            assert torch.isnan(a[t]).all() and torch.isnan(b[t]).all(), f"{what}: storage {f} row {t} written"
                # the storage row holds the call's own outputs
                assert torch.equal(s1["actions"][store_row], o1["actions"]) and torch.equal(s1["mu"][store_row], o1["mu"])
                assert torch.equal(s1["values"][store_row].flatten(), o1["values"].flatten())
                assert torch.equal(s1["actions_log_prob"][store_row].flatten(), o1["logp"])
                assert torch.equal(s1["observations"][store_row], obs) and torch.equal(s1["privileged_observations"][store_row], priv)
                assert torch.equal(s1["observation_histories"][store_row], hist)


@pytest.mark.parametrize("n", [33, 95, 160])
def test_without_a_store(n, monkeypatch):
    ac = _net(42)
    obs, priv, hist, eps = _inputs(n, 42)
    o1, o0 = _both(monkeypatch, lambda: _act(ac, obs, priv, hist, None, 64, None, 0))
    for k in o1:
        assert not torch.isnan(o1[k]).any() and torch.equal(o1[k], o0[k]), k


@pytest.mark.parametrize("n", [33, 95, 160])
def test_only_actions_requested(n, monkeypatch):
    """mu, values and logp NULL: the actions and the storage row are written, the other outputs stay untouched (NaN)."""
    from lrl.ppo.rollout_storage import RolloutStorage
    ac = _net(42)
    obs, priv, hist, eps = _inputs(n, 42)
    st = RolloutStorage(n, T, [42], [18], [630], [NA], DEV)

    def call():
        out = _act(ac, obs, priv, hist, eps, 0, st, 1, want=("actions",))
        return out, {f: getattr(st, f)[1].clone() for f in FIELDS}
    (o1, s1), (o0, s0) = _both(monkeypatch, call)
    assert not torch.isnan(o1["actions"]).any() and torch.equal(o1["actions"], o0["actions"])
    for k in ("mu", "values", "logp"):
        assert torch.isnan(o1[k]).all() and torch.isnan(o0[k]).all(), k
    for f in FIELDS:
        assert not torch.isnan(s1[f]).any() and torch.equal(s1[f], s0[f]), f
    full = _act(ac, obs, priv, hist, eps, 0, None, 0)  # the values and log-probs in storage are the full call's
    assert torch.equal(s1["values"].flatten(), full["values"].flatten())
    assert torch.equal(s1["actions_log_prob"].flatten(), full["logp"]) and torch.equal(s1["mu"], full["mu"])


def test_a_net_outside_the_envelope_takes_the_chain(monkeypatch):
    """ac_h0 = 1024: H1's planes (32 x 1024 x 6 B) do not fit the kernel's LDS, so both settings run the GEMM chain and
    agree trivially; the result is the chain's (held against torch within the fp32 bar of test_ppo_gpu)."""
    from lrl.ppo.actor_critic import AC_Args, ActorCritic
    monkeypatch.setattr(AC_Args, "actor_hidden_dims", [1024, 256, 128])
    monkeypatch.setattr(AC_Args, "critic_hidden_dims", [1024, 256, 128])
    n, no = 95, 42
    ac = ActorCritic(no, 18, 15 * no, NA)
    init_params(ac)
    ac = ac.cuda()
    obs, priv, hist, eps = _inputs(n, no)
    o1, o0 = _both(monkeypatch, lambda: _act(ac, obs, priv, hist, eps, 0, None, 0))
    for k in o1:
        assert not torch.isnan(o1[k]).any() and torch.equal(o1[k], o0[k]), k
    with torch.no_grad():
        ac.update_distribution(obs, priv)
        torch.testing.assert_close(o1["mu"], ac.action_mean, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(o1["values"], ac.evaluate(obs, priv), rtol=1e-4, atol=1e-4)
