"""lrl_ppo_act_shift: the rollout act that, while copying the history rows into the rollout storage, also shifts them
left by one observation in place (copy_rows_shift of csrc/lrl_ppo.hip), on both act paths — the one-launch kernel
(LRL_ACT_FUSED=1) and the GEMM chain's head kernel (LRL_ACT_FUSED=0), forced as tests/test_act_onelaunch_gpu.py does.

hist[r][c] = r * 1024 + c, exact in float32 and unique to (r, c) for the widths used here (c < 1024): a load overtaken
by another thread's shifted store, or a wrong row, shows up as a wrong number.

Row counts: 64 (whole tiles), 80 (the one-launch kernel's last 32-row tile holds 16 rows: the actor's workgroup copies
all of them, the critic's none), 88 (24 rows: the critic's half is partly full, 8 of 16), 97 (a last tile of one row),
2048 (128 head-kernel workgroups; the default path's first one-launch size).
History shapes (num_obs, H): the presets' (42, 630); (42, 84), a shift by half the row; (42, 42), where nothing moves
and nothing may be written; (235, 705), an odd observation width the act's envelope admits (the perceptive net's, as in
test_act_onelaunch_gpu.py), so that the scalar branch of the copy runs — 705 floats do not fit a float2 row.
"""
import ctypes as C

import pytest
import torch

from helpers import init_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NA = 12
T = 2  # storage rows
PAD = 40  # rows of the history allocation beyond n
FIELDS = ("observations", "privileged_observations", "observation_histories", "actions", "mu", "sigma", "values",
          "actions_log_prob")
SHAPES = ((42, 630), (42, 84), (42, 42), (235, 705))

_nets = {}


def _net(no, H):
    if (no, H) not in _nets:
        from lrl.ppo.actor_critic import ActorCritic
        ac = ActorCritic(no, 18, H, NA)
        init_params(ac)
        ac = ac.cuda()
        with torch.no_grad():
            ac.std.copy_(torch.linspace(0.5, 1.5, NA))
        _nets[(no, H)] = ac
    return _nets[(no, H)]


def _history(n, H):
    r = torch.arange(n + PAD, device=DEV, dtype=torch.float32)[:, None]
    c = torch.arange(H, device=DEV, dtype=torch.float32)[None]
    h = r * 1024 + c
    assert H <= 1024 and float(h.max()) < 2 ** 24
    return h.contiguous()


def _act(ac, obs, priv, hist, n, st, store_row, shift, slot):
    """One act on NaN-filled outputs and storage; the shifting entry point when `shift`."""
    from lrl import _abi
    net = ac.flatten_parameters()
    L = _abi.lib()
    nbytes = L.lrl_ppo_act_workspace_bytes(C.byref(net), n)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    out = {"actions": torch.full((n, NA), float("nan"), device=DEV), "mu": torch.full((n, NA), float("nan"), device=DEV),
           "values": torch.full((n, 1), float("nan"), device=DEV), "logp": torch.full((n,), float("nan"), device=DEV)}
    for f in FIELDS:
        getattr(st, f).fill_(float("nan"))
    args = (net, ac._flat.data_ptr(), obs.data_ptr(), priv.data_ptr(), hist.data_ptr(), n, None, 11, 3, 0,
            out["actions"].data_ptr(), out["mu"].data_ptr(), out["values"].data_ptr(), out["logp"].data_ptr(),
            st.store_desc(), store_row, ws.data_ptr(), _abi.stream_of(torch.device(DEV)))
    if shift:
        _abi.check(L.lrl_ppo_act_shift(*args, hist.data_ptr(), slot))
    else:
        _abi.check(L.lrl_ppo_act(*args))
    torch.cuda.synchronize()
    out.update({"store/" + f: getattr(st, f).clone() for f in FIELDS})
    return out


@pytest.mark.parametrize("n", [64, 80, 88, 97, 2048])
@pytest.mark.parametrize("no,H", SHAPES)
@pytest.mark.parametrize("fused", ["1", "0"])
def test_act_shifts_the_history_it_stores(fused, no, H, n, monkeypatch):
    from lrl.ppo.rollout_storage import RolloutStorage
    monkeypatch.setenv("LRL_ACT_FUSED", fused)
    ac = _net(no, H)
    g = torch.Generator(device=DEV).manual_seed(5)
    obs, priv = (torch.randn(n, k, device=DEV, generator=g) for k in (no, 18))
    orig = _history(n, H)
    st = RolloutStorage(n, T, [no], [18], [H], [NA], DEV)
    store_row = 1
    plain_hist = orig.clone()
    plain = _act(ac, obs, priv, plain_hist, n, st, store_row, False, no)
    assert torch.equal(plain_hist, orig), "lrl_ppo_act wrote to its history"
    hist = orig.clone()
    got = _act(ac, obs, priv, hist, n, st, store_row, True, no)
    what = f"fused={fused} no={no} H={H} n={n}"
    # the storage row holds the row as it was; the history is shifted, its newest slot and the rows past n untouched
    assert torch.equal(got["store/observation_histories"][store_row], orig[:n]), f"{what}: stored history"
    assert torch.equal(hist[:n, : H - no], orig[:n, no:]), f"{what}: shifted part"
    assert torch.equal(hist[:n, H - no:], orig[:n, H - no:]), f"{what}: newest slot written"
    assert torch.equal(hist[n:], orig[n:]), f"{what}: rows past n written"
    # everything else as the call without the shift: outputs, the storage row, and NaN in the other storage row
    for k in plain:
        a, b = got[k], plain[k]
        if k.startswith("store/"):
            assert not torch.isnan(a[store_row]).any(), f"{what}: {k} has skipped rows"
            assert torch.equal(a[store_row], b[store_row]), f"{what}: {k}"
            assert torch.isnan(a[1 - store_row]).all(), f"{what}: {k} written outside its row"
        else:
            assert not torch.isnan(a).any() and torch.equal(a, b), f"{what}: {k}"


def test_the_shift_needs_its_own_history_a_store_and_a_dividing_slot():
    """Refused without a launch: hist_shift other than hist, no store, a slot width that does not divide hist_dim."""
    from lrl import _abi
    from lrl.ppo.rollout_storage import RolloutStorage
    n, no, H = 64, 42, 630
    ac = _net(no, H)
    net = ac.flatten_parameters()
    L = _abi.lib()
    ws = torch.empty(max(L.lrl_ppo_act_workspace_bytes(C.byref(net), n), 16), dtype=torch.uint8, device=DEV)
    obs, priv = torch.zeros(n, no, device=DEV), torch.zeros(n, 18, device=DEV)
    hist, other = _history(n, H), _history(n, H)
    orig = hist.clone()
    st = RolloutStorage(n, T, [no], [18], [H], [NA], DEV)
    out = torch.empty(n, NA, device=DEV)

    def call(store, shift, slot):
        return L.lrl_ppo_act_shift(net, ac._flat.data_ptr(), obs.data_ptr(), priv.data_ptr(), hist.data_ptr(), n, None,
                                   11, 3, 0, out.data_ptr(), None, None, None, store, 0, ws.data_ptr(),
                                   _abi.stream_of(torch.device(DEV)), shift, slot)
    assert call(st.store_desc(), other.data_ptr(), no) == -1
    assert call(None, hist.data_ptr(), no) == -1
    assert call(st.store_desc(), hist.data_ptr(), 0) == -1
    assert call(st.store_desc(), hist.data_ptr(), 40) == -1
    torch.cuda.synchronize()
    assert torch.equal(hist, orig)
    assert call(st.store_desc(), None, 0) == 0  # hist_shift NULL: lrl_ppo_act
    torch.cuda.synchronize()
    assert torch.equal(hist, orig)
