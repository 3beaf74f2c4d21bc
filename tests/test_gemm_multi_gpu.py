"""The multi-problem GEMM launch (gemm_launch_multi of csrc/lrl_gemm.hip, through lrl_gemm_f32_multi) and its use in
the backward tail of lrl_ppo_forward_backward (LRL_PPO_BWD_MULTI).

Every comparison is exact: a multi launch must leave, in every output buffer and every workspace (the split-k partials
and the bias partials behind them), the bits that separate lrl_gemm_f32_ex launches of the same descriptors leave from
the same inputs.  Outputs and workspaces sit between guard regions and start out as a sentinel bit pattern, so a job
that writes outside its own C / partials fails the comparison (and the guard check).  The descriptors of a set are
given in grid order: riders first, the host (the large weight gradient) last."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import pytest
import torch

from helpers import init_params
from lrl import _abi

pytestmark = pytest.mark.gpu
dev = "cuda:0"
NN, TN = 2, 3
DELU, PARTIAL = 3, 4
GUARD = 1024                 # floats of guard on each side of an output (keeps the 16-byte alignment)
SENT = 0x7FA5A5A5            # a NaN with a payload no kernel produces
MAX_SPLITS = 8               # workspace room (the update's split count for these shapes is at most 4)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tn(M, N, K, groups=1, gather=0, expect=None):
    """Weight gradient in the update's form: dY [K][groups * M] and X [K][groups * N] (group offsets are column offsets
    inside the row pitch); gather: X is a `gather`-row buffer read through a random row list."""
    return NS(layout=TN, epi=PARTIAL, M=M, N=N, K=K, groups=groups, gather=gather, expect=expect)


def nn(M, N, K, lda=None, expect=None):
    """Backward-data product with the ELU' epilogue: dY [M][K] (pitch lda), W [K][N], aux [M][N]."""
    return NS(layout=NN, epi=DELU, M=M, N=N, K=K, groups=1, gather=0, lda=lda or K, expect=expect)


def _inputs(j, g):
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    if j.layout == TN:
        j.A = rn(j.K, j.groups * j.M)
        j.B = rn(j.gather or j.K, j.groups * j.N)
        j.rows = torch.randperm(j.gather, device=dev, generator=g)[:j.K].contiguous() if j.gather else None
        j.aux = None
        j.c_len, j.ws_len, j.db_len = j.groups * j.M * j.N, MAX_SPLITS * j.groups * (j.M * j.N + j.M), j.groups * j.M
    else:
        j.A = rn(j.M, j.lda)
        j.B = rn(j.K, j.N)
        j.aux = rn(j.M, j.N)   # both signs: both branches of elu'
        j.rows = None
        j.c_len, j.ws_len, j.db_len = j.M * j.N, 0, 0
    return j


def _arena(n):
    """n floats between two guards, all sentinel; returns (whole arena as int32, the inner float view)."""
    a = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
    return a, a.view(torch.float32)[GUARD:GUARD + n]


def _desc(j):
    """A descriptor of job j on fresh sentinel outputs; returns (desc, arenas, path, splits)."""
    arenas = {k: _arena(n) for k, n in (("C", j.c_len), ("ws", j.ws_len), ("db", j.db_len)) if n}
    path, splits = C.c_int32(-1), C.c_int32(-1)
    d = _abi.LrlGemmDesc()
    d.layout, d.epi, d.M, d.N, d.K, d.groups, d.planes, d.splits = j.layout, j.epi, j.M, j.N, j.K, j.groups, 0, 0
    d.A, d.B, d.C = j.A.data_ptr(), j.B.data_ptr(), arenas["C"][1].data_ptr()
    d.lda, d.ldb = j.A.stride(0), j.B.stride(0)
    if j.layout == TN:
        d.ga, d.gb, d.ldc = j.M, j.N, j.N
        d.rows = j.rows.data_ptr() if j.rows is not None else None
        d.workspace, d.workspace_floats = arenas["ws"][1].data_ptr(), j.ws_len
        d.bias = arenas["db"][1].data_ptr()
    else:
        d.ldc, d.aux, d.ld_aux = j.N, j.aux.data_ptr(), j.N
    d.path_out, d.splits_out = C.pointer(path), C.pointer(splits)
    return d, arenas, path, splits


def _guards_intact(arenas):
    return all(bool((a[:GUARD] == SENT).all()) and bool((a[-GUARD:] == SENT).all()) for a, _ in arenas.values())


def _report(path):
    v = path.value
    return (_abi.GEMM_FAMILIES.get(v & 0xff), (v >> 8) & 0xff, (v >> 16) & 0xff, bool(v >> 24 & 1))


def _multi(descs):
    arr = (_abi.LrlGemmDesc * len(descs))(*descs)
    rc = _abi.lib().lrl_gemm_f32_multi(arr, C.c_int32(len(descs)), _stream())
    torch.cuda.synchronize()
    return rc


HOST_A = dict(M=128, N=256, K=512, groups=2)   # x6t, 128-wide n tile
# name -> jobs in grid order (riders, then the host).  The first three are the smallest shapes that reach each body and
# edge; b-128 is combination B at the smallest row count at which the dispatcher gives the NN rider its 128-row tile
# (512 workgroups: the benchmark minibatch's kernel); u-* are the products of the Mini Cheetah update at a 256-row
# minibatch, which the update-level test below relies on being carried by the multi launches.
SETS = {
    "a": [tn(18, 128, 512, expect=("x6", 64, 128, False)), nn(500, 128, 18, lda=32, expect=("staged", 64, 64, False)),
          tn(**HOST_A, expect=("x6t", 128, 128, False))],
    "b": [tn(128, 256, 512, expect=("x6t", 128, 128, False)), nn(512, 256, 128, expect=("x6", 64, 64, True)),
          tn(128, 64, 512, expect=("x6t", 128, 64, False))],
    "c": [tn(256, 18, 512, gather=2048, expect=("x6", 128, 64, False)), tn(**HOST_A, expect=("x6t", 128, 128, False))],
    "b-128": [tn(128, 256, 512, expect=("x6t", 128, 128, False)), nn(16384, 256, 128, expect=("x6", 128, 64, True)),
              tn(128, 64, 512, expect=("x6t", 128, 64, False))],
    "u-a": [tn(18, 128, 256), nn(256, 128, 18, lda=32), tn(128, 256, 256, groups=2)],
    "u-b": [tn(128, 256, 256), nn(256, 256, 128), tn(256, 512, 256, groups=2)],
    "u-b2": [tn(128, 256, 256), nn(256, 256, 128), tn(1024, 60, 256)],
    "u-c": [tn(256, 18, 256, gather=1024), tn(1024, 60, 256)],
    "u-c2": [tn(256, 18, 256, gather=1024), tn(256, 512, 256, groups=2)],
    "riders-b": [tn(128, 256, 512), nn(512, 256, 128)],
}


def _jobs(name):
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, name)))
    jobs = [_inputs(NS(**vars(j)), g) for j in SETS[name]]
    for j in jobs:
        if j.layout == TN and j.N == 60:   # the actor / critic input: 60 columns at the pitch of 64
            j.B = torch.randn(j.K, 64, device=dev, generator=g)[:, :60]
    return jobs


@pytest.mark.parametrize("name", list(SETS))
def test_multi_launch_is_bit_identical_to_separate_launches(name):
    """C, the split-k partials and the bias partials (the whole workspace), db and the split counts of every job of a
    set: the multi launch against one lrl_gemm_f32_ex launch per job; guards untouched; the dispatcher's family and
    tile for each job alone is the one its combination is built from."""
    jobs = _jobs(name)
    sep = []
    for j in jobs:
        d, arenas, path, splits = _desc(j)
        _abi.check(_abi.lib().lrl_gemm_f32_ex(C.byref(d), _stream()))
        torch.cuda.synchronize()
        assert _guards_intact(arenas)
        if j.expect:
            assert _report(path) == j.expect
        sep.append((arenas, path.value, splits.value))
    mul = [_desc(j) for j in jobs]
    assert _multi([m[0] for m in mul]) == 0, _abi.lib().lrl_last_error()
    for j, (arenas_s, path_s, splits_s), (_, arenas_m, path_m, splits_m) in zip(jobs, sep, mul):
        assert _guards_intact(arenas_m)
        assert splits_m.value == splits_s
        for k in arenas_s:
            assert torch.equal(arenas_m[k][0], arenas_s[k][0]), (name, j.layout, j.M, j.N, k)
        inner = arenas_m["C"][0][GUARD:-GUARD]
        assert not bool((inner == SENT).any())   # every element of C was written
    assert mul[-1][2].value == sep[-1][1]        # the path report is the host's


@pytest.mark.parametrize("order", [(2, 0, 1), (2, 2), (0, 2), (1, 2), (0, 1)])
def test_sets_outside_the_combinations_launch_nothing(order):
    """Jobs of set "a" in an order / selection that is no combination (the host first, two hosts, one rider short, the
    riders alone): the call reports "not eligible" and leaves every output and workspace as it found them."""
    jobs = _jobs("a")
    descs = [_desc(jobs[i]) for i in order]
    assert _multi([d[0] for d in descs]) == _abi.GEMM_MULTI_NOT_ELIGIBLE
    for _, arenas, _, _ in descs:
        assert all(bool((a == SENT).all()) for a, _ in arenas.values())


def test_fp32_paths_are_not_eligible():
    """With the bf16-split families switched off (lrl_debug_gemm_paths bit 4) every job dispatches to an fp32 family
    that no multi kernel carries: the caller's one-by-one fallback."""
    jobs = _jobs("a")
    descs = [_desc(j) for j in jobs]
    prev = _abi.lib().lrl_debug_gemm_paths(C.c_int32(16))
    try:
        rc = _multi([d[0] for d in descs])
    finally:
        _abi.lib().lrl_debug_gemm_paths(C.c_int32(prev))
    assert rc == _abi.GEMM_MULTI_NOT_ELIGIBLE
    for _, arenas, _, _ in descs:
        assert all(bool((a == SENT).all()) for a, _ in arenas.values())


# ---- the update ------------------------------------------------------------------------------------------------------
class _Env:
    """Environment switches the library reads at every call, restored on exit."""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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
        st.actions_log_prob.copy_(-11.0 + rn(st.values))


def _forward_backward(alg, ac, mb, rows, hist_ld, env):
    """grads, ctrl and the workspace (as int32) after one lrl_ppo_forward_backward under the switches `env`."""
    nst = alg._native_state(mb)
    net, hp, grads, ctrl, ws = nst["net"], nst["hp"], nst["grads"], nst["ctrl"], nst["ws"]
    s = alg.storage
    fl = lambda t: t.flatten(0, 1)
    batch = _abi.LrlPpoBatch()
    for k, t in dict(obs=s.observations, priv=s.privileged_observations, hist=s.observation_histories,
                     actions=s.actions, values=s.values, returns=s.returns, logp=s.actions_log_prob,
                     adv=s.advantages, mu=s.mu, sigma=s.sigma).items():
        setattr(batch, k, fl(t).data_ptr())
    batch.rows, batch.batch, batch.hist_ld = rows.data_ptr(), mb, hist_ld
    p = lambda t: C.c_void_p(t.data_ptr())
    grads.fill_(float("nan"))
    # (the workspace is uninitialised memory to the library: it writes whatever it reads, so nothing of an earlier
    # run needs to survive)
    ws.view(torch.uint8)[:ws.numel() * ws.element_size() // 4 * 4].view(torch.int32).fill_(SENT)
    with _Env(**env):
        _abi.check(_abi.lib().lrl_ppo_forward_backward(C.byref(net), p(ac._flat), p(grads), C.byref(batch),
                                                       C.byref(hp), p(ws), p(ctrl), _stream()))
        torch.cuda.synchronize()
    as_bits = lambda t: t.view(torch.uint8).clone()
    mbs = ctrl.view(torch.float32)[8:12]   # lrl_ppo_ctrl.mb
    return NS(grads=as_bits(grads), ctrl=as_bits(mbs), ws=as_bits(ws), net=net, raw=grads.clone())


SWITCHES = [dict(LRL_PPO_BWD_MULTI="0", LRL_PPO_FORK=None), dict(LRL_PPO_BWD_MULTI="0", LRL_PPO_FORK="0"),
            dict(LRL_PPO_BWD_MULTI="2", LRL_PPO_FORK=None), dict(LRL_PPO_BWD_MULTI="3", LRL_PPO_FORK=None),
            dict(LRL_PPO_BWD_MULTI=None, LRL_PPO_FORK=None)]


@pytest.mark.parametrize("num_obs,history,N,T", [(42, 630, 256, 4), (42, 630, 200, 4), (235, 3525, 256, 4)])
def test_update_gradients_do_not_depend_on_the_backward_packing(num_obs, history, N, T):
    """The packed backward tail (LRL_PPO_BWD_MULTI=1, and unset) leaves the same bits as the eight-launch path with and
    without its stream fork — the whole flat gradient, ctrl's mb slots and the whole workspace, the dhe1 / dhe2 rows and
    every partial slice included.  All settings launch the one collected job list, so the cases are the shapes at which
    the ways of launching it can part: the Mini Cheetah preset net at a 256-row minibatch; at 200 rows (the last head
    workgroup partial, row counts off the 64 / 128-row tiles, so jobs may fall out of the packed sets into launch_jobs'
    one-by-one path); and the perceptive net (X pitch 256, the history padded 3525 -> 3536)."""
    from lrl.ppo.actor_critic import ActorCritic
    from lrl.ppo.ppo import PPO
    ac = ActorCritic(num_obs, 18, history, 12)
    init_params(ac)
    alg = PPO(ac.cuda(), device=dev, fused=True)
    alg.init_storage(N, T, [num_obs], [18], [history], [12])
    _random_storage(alg)
    mb = N * T // 4
    assert mb == N
    rows = torch.randperm(N * T, device=dev, generator=torch.Generator(device=dev).manual_seed(7))[:mb].contiguous()
    hist_ld = alg.storage.observation_histories.flatten(0, 1).stride(0)
    ref = _forward_backward(alg, ac, mb, rows, hist_ld, dict(LRL_PPO_BWD_MULTI="1", LRL_PPO_FORK=None))
    n = ref.net
    for off in (n.e1w, n.e2w, n.e3w, n.w1, n.w2, n.w3):   # the tail's gradients were written, and are not all zero
        seg = ref.raw[off:off + 16]
        assert bool(torch.isfinite(seg).all()) and bool(seg.abs().sum() > 0)
    for env in SWITCHES:
        got = _forward_backward(alg, ac, mb, rows, hist_ld, env)
        for k in ("grads", "ctrl", "ws"):
            assert torch.equal(getattr(got, k), getattr(ref, k)), (env, k)


def test_plain_net_runs_through_the_fallback():
    """The navigation policy's plain tanh net has no encoder chain to pack: its forward / backward gives the same bits
    under every setting of the switch."""
    from lrl.hlp import PPO, ActorCritic
    NO, NP, NH, NA = 14, 18, 16, 3
    N, T = 37, 20
    ac = ActorCritic(NO, NP, NH, NA)
    init_params(ac)
    ac = ac.cuda()
    alg = PPO(ac, device=dev, fused=True)
    alg.init_storage(N, T, [NO], [NP], [NH], [NA])
    _random_storage(alg)
    with torch.no_grad():
        alg.storage.actions_log_prob.add_(6.7)   # near the 3-action policy's own log-probs
    mb = N * T // 4
    rows = torch.randperm(N * T, device=dev, generator=torch.Generator(device=dev).manual_seed(7))[:mb].contiguous()
    ref = _forward_backward(alg, ac, mb, rows, NH, dict(LRL_PPO_BWD_MULTI="1", LRL_PPO_FORK=None))
    assert ref.net.plain == 1
    assert bool(torch.isfinite(ref.raw[ref.net.w1:ref.net.w1 + 16]).all())
    for env in SWITCHES[:1] + SWITCHES[-1:]:
        got = _forward_backward(alg, ac, mb, rows, NH, env)
        for k in ("grads", "ctrl", "ws"):
            assert torch.equal(getattr(got, k), getattr(ref, k)), (env, k)
