"""The two inference entry points, lrl_ppo_act_student and lrl_ppo_act, through ctypes against the float64 restatement
and its error bound (tests/act_ref.py), at the row counts and history forms that switch the GEMM family:

  rows      1, 31 / 32 / 33, 63 / 64 / 65, 127 / 128 / 129, 256 / 257: pick_tile's 32 / 64 / 128 edges, X6_MIN_M = 64,
            glds_fits' multiples of 64 and thin_fits' 256 (the perceptive net runs 1, 33, 64, 65, 257);
  nets      (num_obs, num_hist) = (42, 630), (48, 720) — hist_pad(720) == 720, the third branch of
            adaptation_l1_forward — and the perceptive (235, 3525) with X at pitch 256;
  history   1 contiguous with hist_ld = 0;  2 contiguous with hist_ld = num_hist;  3 pitch hist_pad(num_hist) on a
            16-byte aligned base with zero padding (the padded form: pad_cols_kernel, k = hist_pad), also as the
            RolloutStorage's own buffer ("3s");  4 the same pitch, base one float into the buffer (misaligned: the
            unpadded form);  5 pitch num_hist + 2;  6 pitch hist_pad(num_hist) + 1.

Every call runs on NaN-filled outputs and a workspace of exactly *_workspace_bytes followed by a 4 KB NaN guard in the
same allocation; afterwards the guard is all NaN, no output holds a NaN, and obs / priv / hist (padding and the rows
around it included) / eps / the parameters have the bits they had before.  The history buffers carry one row before
row 0 and one behind the last, so a read a few floats outside the rows stays inside the allocation and shows as NaN.

A defect of the library each test fails on.  The first three were put into scratch builds of the library and run on
an MI355X (never committed); the rest are read off the float64 restatement of the defect against the bound
(tests/test_act_ref.py::test_listed_defects_move_an_output_by_ten_bounds) or off the assertion itself.
  * pad_cols_kernel leaving the padding columns of the re-pitched Wd1 unwritten: test_student_act_within_float64_bound
    fails at its first padded call (42x630, n = 1, form 3: the mean is NaN, from the workspace's fill), and so does
    test_history_padding_is_never_used.
  * layers_of(net, true) taking two groups: test_student_act_within_float64_bound fails at 42x630 n = 31 (the mean 17
    times the first form of the bound out, 100 times more in today's), test_student_reads_only_the_actors_half at
    n = 33 (NaN in the mean).  At n = 1 the second group only writes behind the one row, inside the workspace, and
    both outputs are right: nothing here sees that.
  * the staged kernel's k tail (Stager::load) reading a whole float4 past K: test_student_act_within_float64_bound
    fails at n = 1 and 33 on forms 1 and 2 (the two floats behind a row are the next row's, behind the last the NaN
    row: NaN in the mean); on forms 3 - 6 with zero padding the outputs are right, and
    test_history_padding_is_never_used fails there with NaN padding (form 4, n = 1).  From 64 rows the products run
    on gemm_x6_kernel and the defect is not executed.
  test_student_reads_only_the_actors_half   also: a student head that reads std, the encoder or the critic's head
  test_teacher_reads_nothing_of_the_adaptation_module   a plane job or a copy that runs over adapt_begin
  test_student_without_a_latent_buffer      the latent copy running on a NULL pointer or over n + 1 rows
  test_wrapper_equals_the_ctypes_call       act_student_fused passing hist.shape[1] for the pitch; _student_ws kept
                                            at the first call's size
  test_student_refusals                     the hist_ld check dropped (rows read at a pitch below their width)
  test_teacher_act_within_float64_bound     X's last float4 dropped from body 1 (48 - 121 bounds in mu), a bias of the
                                            last hidden layer lost for a row (17 - 24), the latent a column late (128 -
                                            330), std read reversed (2e4 in actions)
  test_teacher_store_row_equals_outputs     the head's store writing row store_row at pitch 16 instead of n
  test_trained_weights_within_bound         the same defects on weights that are not uniform (not restated in float64
                                            for these weights: the figures above are the init_params nets')

The accuracy tests print, per output, the worst error / bound of the native call and, for the (42, 630) net, of torch's
own fp32 modules on the GPU with TF32 off (measurements: profiles/act_rows_error_ratios.txt).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import act_ref as R
from helpers import npy, same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NA = R.NUM_ACTIONS
NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257)
NS_PERCEPTIVE = (1, 33, 64, 65, 257)
NS_EDGE = (1, 33, 64, 65, 257)
NMAX = 257
GUARD = 4096
NAN = float("nan")
INVALID = -1  # LRL_E_INVALID

NET_N = [pytest.param(net, n, id=f"{net[0]}x{net[1]}-{n}") for net in R.NETS
         for n in (NS_PERCEPTIVE if net[0] == 235 else NS)]
NET_EDGE = [pytest.param(net, n, id=f"{net[0]}x{net[1]}-{n}") for net in R.NETS for n in NS_EDGE]
NET_IDS = [f"{no}x{nh}" for no, nh in R.NETS]
_cases = {}


class Case:
    """One net on the GPU, its 257 input rows and the float64 reference of both acts over them (rows are independent:
    the reference of the first n rows is the first n rows of the reference)."""

    def __init__(self, net):
        if net == "trained":
            ac, g = R.trained_net()
            rows = R.trained_rows(g, NMAX)
            self.no, self.nh = 42, 630
        else:
            ac, rows = R.make_net(*net), R.inputs(*net, NMAX)
            self.no, self.nh = net
        self.name = net if net == "trained" else f"{net[0]}x{net[1]}"
        P = R.params_of(ac)
        self.student = R.student_ref(P, rows[0], rows[2])
        self.teacher = R.teacher_ref(P, rows[0], rows[1], rows[3])
        self.ac = ac.cuda()
        self.net = self.ac.flatten_parameters()
        self.obs, self.priv, self.hist, self.eps = (torch.from_numpy(a).to(DEV) for a in rows)


def case(net):
    if net not in _cases:
        _cases[net] = Case(net)
    return _cases[net]


def first(ref, n):
    return {k: v[:n] for k, v in ref.items()}


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32).clone()


class Unchanged:
    """The bits of the given tensors, taken now; check() compares them with the tensors' bits then."""

    def __init__(self, **tensors):
        self.t = tensors
        self.b = {k: bits(v) for k, v in tensors.items()}

    def check(self, what):
        for k, v in self.t.items():
            assert torch.equal(bits(v), self.b[k]), f"{what}: {k} was written"


def workspace(nbytes):
    """(buffer of nbytes + GUARD bytes, all NaN; its guard)"""
    assert nbytes >= 0 and nbytes % 4 == 0
    buf = torch.full(((nbytes + GUARD) // 4,), NAN, device=DEV)
    return buf, buf[nbytes // 4:]


def hist_pad(h):
    return (h + 15) // 16 * 16


def hist_form(form, H, pad=0.0, edge=NAN):
    """The rows H [n][num_hist] laid out as history form `form`: (the whole buffer, the [n][num_hist] view of the rows
    in it, the hist_ld argument).  Columns from num_hist to the pitch hold `pad`; one row in front of row 0 and one
    behind the last (and the floats in front of a shifted base) hold `edge`."""
    n, nh = H.shape
    hp = hist_pad(nh)
    if form == "3s":  # the rollout storage's own buffer: its rows are the whole allocation
        from lrl.ppo.rollout_storage import RolloutStorage
        st = RolloutStorage(n, 1, [1], [R.NUM_PRIV], [nh], [NA], DEV)  # (its other buffers are not used)
        buf, view = st._hist_padded, st.observation_histories[0]
        assert view.stride(0) == hp and view.data_ptr() % 16 == 0
        buf[0, :, nh:] = pad
        view.copy_(H)
        return buf, view, hp
    ld, off = {1: (nh, 0), 2: (nh, 0), 3: (hp, 0), 4: (hp, 1), 5: (nh + 2, 0), 6: (hp + 1, 0)}[form]
    buf = torch.full((off + (n + 2) * ld,), edge, device=DEV)
    rows = buf[off + ld:off + ld + n * ld].view(n, ld)
    rows[:, nh:] = pad
    view = rows[:, :nh]
    view.copy_(H)
    if form == 3:
        assert view.data_ptr() % 16 == 0
    if form == 4:
        assert view.data_ptr() % 16 == 4
    return buf, view, (0 if form == 1 else ld)


def forms_of(c):
    """(for a history width that is a multiple of 16, forms 3 and 4 are form 2)"""
    f = (1, 2, 3, 4, 5, 6) if c.nh % 16 else (1, 2, 5, 6)
    return f + ("3s",) if c.name == "42x630" else f


def student(c, obs, hview, hist_ld, n, params=None, latent=True, out_rows=None, buf=None):
    """lrl_ppo_act_student on the n rows of obs / hview.  Returns {"mean", "latent"} as numpy ([out_rows][.], default
    n rows; latent None when not asked for), after the checks every call gets."""
    from lrl import _abi
    L = _abi.lib()
    out_rows = n if out_rows is None else out_rows
    params = c.ac._flat if params is None else params
    nbytes = L.lrl_ppo_act_student_workspace_bytes(C.byref(c.net), n)
    ws, guard = workspace(nbytes)
    mean = torch.full((out_rows, NA), NAN, device=DEV)
    lat = torch.full((out_rows, c.net.latent), NAN, device=DEV) if latent else None
    keep = Unchanged(obs=obs, hist=hview if buf is None else buf, params=params)
    _abi.check(L.lrl_ppo_act_student(c.net, params.data_ptr(), obs.data_ptr(), hview.data_ptr(), hist_ld, n,
                                     mean.data_ptr(), lat.data_ptr() if latent else None, ws.data_ptr(),
                                     _abi.stream_of(DEV)))
    torch.cuda.synchronize()
    what = f"student {c.name} n={n} hist_ld={hist_ld}"
    assert torch.isnan(guard).all(), f"{what}: wrote behind its workspace"
    keep.check(what)
    out = {"mean": npy(mean), "latent": npy(lat) if latent else None}
    for k, v in out.items():
        if v is not None:
            assert not np.isnan(v[:n]).any(), f"{what}: {k} holds NaN"
            assert np.isnan(v[n:]).all(), f"{what}: {k} written behind row n"
    return out


def teacher(c, n, obs, priv, hist, eps, params=None, st=None, store_row=0):
    """lrl_ppo_act with injected noise on n rows.  Returns the four outputs as numpy."""
    from lrl import _abi
    L = _abi.lib()
    params = c.ac._flat if params is None else params
    ws, guard = workspace(L.lrl_ppo_act_workspace_bytes(C.byref(c.net), n))
    out = {"actions": torch.full((n, NA), NAN, device=DEV), "mu": torch.full((n, NA), NAN, device=DEV),
           "values": torch.full((n, 1), NAN, device=DEV), "logp": torch.full((n,), NAN, device=DEV)}
    keep = Unchanged(obs=obs, priv=priv, hist=hist, eps=eps, params=params)
    _abi.check(L.lrl_ppo_act(c.net, params.data_ptr(), obs.data_ptr(), priv.data_ptr(), hist.data_ptr(), n,
                             eps.data_ptr(), 11, 3, 0, out["actions"].data_ptr(), out["mu"].data_ptr(),
                             out["values"].data_ptr(), out["logp"].data_ptr(),
                             st.store_desc() if st is not None else None, store_row, ws.data_ptr(),
                             _abi.stream_of(DEV)))
    torch.cuda.synchronize()
    what = f"teacher {c.name} n={n}"
    assert torch.isnan(guard).all(), f"{what}: wrote behind its workspace"
    keep.check(what)
    out = {k: npy(v) for k, v in out.items()}
    for k, v in out.items():
        assert not np.isnan(v).any(), f"{what}: {k} holds NaN"
    return out


def fused_settings(n):
    """LRL_ACT_FUSED values to run: from X6_MIN_M rows the chain and the one-launch act, below it the chain alone."""
    return ("0", "1") if n >= 64 else (None,)


def report(c, n, form, got, ref, names, torch_out=None):
    """Print and return the worst error / bound per output (and torch-fp32's where given)."""
    r = R.ratios(got, ref, names)
    t = R.ratios(torch_out, ref, names) if torch_out is not None else {}
    for k in names:
        print(f"act_rows n={n} net={c.name} form={form} output={k} native={r[k]:.3e} "
              f"torch_fp32={t[k]:.3e}" if k in t else
              f"act_rows n={n} net={c.name} form={form} output={k} native={r[k]:.3e} torch_fp32=-")
    return r


def torch_student(c, n):
    """torch's own fp32 modules on the same rows (TF32 off)."""
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        with torch.no_grad():
            lat = c.ac.adaptation_module(c.hist[:n])
            mean = c.ac.actor_body(torch.cat((c.obs[:n], lat), -1))
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    return {"mean": npy(mean), "latent": npy(lat)}


def torch_teacher(c, n):
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        with torch.no_grad():
            X = torch.cat((c.obs[:n], c.ac.env_factor_encoder(c.priv[:n])), -1)
            mu, values = c.ac.actor_body(X), c.ac.critic_body(X)
            actions = mu + c.ac.std * c.eps[:n]
            logp = torch.distributions.Normal(mu, mu * 0.0 + c.ac.std).log_prob(actions).sum(-1)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    return {"mu": npy(mu), "actions": npy(actions), "values": npy(values), "logp": npy(logp)}


# ---- a. student act against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n", NET_N)
def test_student_act_within_float64_bound(net, n):
    c = case(net)
    obs, ref = c.obs[:n].contiguous(), first(c.student, n)
    t32 = torch_student(c, n) if c.name == "42x630" else None
    for form in forms_of(c):
        buf, view, ld = hist_form(form, c.hist[:n])
        got = student(c, obs, view, ld, n, buf=buf)
        r = report(c, n, form, got, ref, R.STUDENT_OUT, t32)
        assert max(r.values()) <= 1, (form, r)


# ---- b. padding columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n", NET_EDGE)
def test_history_padding_is_never_used(net, n):
    """Form 3 (k runs over the padding against pad_cols_kernel's zero weight columns): padding at 0 and at 1e30 give
    the same bits.  Forms 4 - 6 (k stops at num_hist): NaN in every padding column and in the rows in front of and
    behind the history give the bits that zeros there give."""
    c = case(net)
    obs = c.obs[:n].contiguous()
    for form in forms_of(c):
        if form in (3, "3s"):
            fills = ((0.0, NAN), (1e30, NAN))
        elif form in (4, 5, 6):
            fills = ((0.0, 0.0), (NAN, NAN))
        else:
            continue
        a, b = (student(c, obs, view, ld, n, buf=buf)
                for buf, view, ld in (hist_form(form, c.hist[:n], pad, edge) for pad, edge in fills))
        for k in R.STUDENT_OUT:
            same(a[k], b[k], f"{c.name} n={n} form {form}: {k}")


# ---- c. only the actor's half ------------------------------------------------------------------------------------
def overwritten(c, regions, seed):
    """A copy of the parameters with the given (offset, length) regions at uniform values in +-1e30."""
    flat = c.ac._flat.clone()
    g = torch.Generator(device=DEV).manual_seed(seed)
    for off, length in regions:
        flat[off:off + length] = (torch.rand(length, device=DEV, generator=g) * 2 - 1) * 1e30
    assert torch.isfinite(flat).all()
    return flat


def teacher_only_regions(net):
    """What the student act must not read: the critic's rows of W1 / W2 / W3 and their biases, the critic's head, the
    encoder and std (offsets of the lrl_ppo_net descriptor)."""
    nx = net.num_obs + net.latent
    reg = []
    for w, b, out, inn in ((net.w1, net.b1, net.ac_h0, nx), (net.w2, net.b2, net.ac_h1, net.ac_h0),
                           (net.w3, net.b3, net.ac_h2, net.ac_h1)):
        reg += [(w + out * inn, out * inn), (b + out, out)]
    reg += [(net.w4c, net.ac_h2), (net.b4c, 1), (net.e1w, net.enc_h0 * net.num_priv), (net.e1b, net.enc_h0),
            (net.e2w, net.enc_h1 * net.enc_h0), (net.e2b, net.enc_h1), (net.e3w, net.latent * net.enc_h1),
            (net.e3b, net.latent), (net.std_off, net.num_actions)]
    return reg


@pytest.mark.parametrize("net", R.NETS, ids=NET_IDS)
def test_student_reads_only_the_actors_half(net):
    """(finite values: body 1 runs k over X's whole pitch, and X's zero columns multiply the first weights of the row
    behind — for the actor's last row, the critic's first)"""
    c = case(net)
    flat = overwritten(c, teacher_only_regions(c.net), 3)
    for n in (1, 33, 65, 257):
        obs = c.obs[:n].contiguous()
        buf, view, ld = hist_form(2, c.hist[:n])
        a, b = student(c, obs, view, ld, n, buf=buf), student(c, obs, view, ld, n, params=flat, buf=buf)
        for k in R.STUDENT_OUT:
            same(a[k], b[k], f"{c.name} n={n}: {k}")


@pytest.mark.parametrize("net", R.NETS, ids=NET_IDS)
def test_teacher_reads_nothing_of_the_adaptation_module(net, monkeypatch):
    c = case(net)
    flat = overwritten(c, [(c.net.adapt_begin, c.net.adapt_end - c.net.adapt_begin)], 4)
    for n in (1, 33, 65, 257):
        rows = tuple(t[:n].contiguous() for t in (c.obs, c.priv, c.hist, c.eps))
        for fused in fused_settings(n):
            if fused is not None:
                monkeypatch.setenv("LRL_ACT_FUSED", fused)
            a, b = teacher(c, n, *rows), teacher(c, n, *rows, params=flat)
            for k in R.TEACHER_OUT:
                same(a[k], b[k], f"{c.name} n={n} fused={fused}: {k}")


# ---- d. latent == NULL -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", R.NETS, ids=NET_IDS)
def test_student_without_a_latent_buffer(net):
    c = case(net)
    for n in (1, 33, 65):
        obs = c.obs[:n].contiguous()
        buf, view, ld = hist_form(1, c.hist[:n])
        a = student(c, obs, view, ld, n, buf=buf, out_rows=n + 1)  # (row n of mean and latent stays NaN: checked there)
        b = student(c, obs, view, ld, n, buf=buf, latent=False)
        assert b["latent"] is None
        same(a["mean"][:n], b["mean"], f"{c.name} n={n}: mean")


# ---- e. the Python wrapper ---------------------------------------------------------------------------------------
def test_wrapper_equals_the_ctypes_call():
    """act_student_fused on hist[n_train:] of a contiguous history (odd n_train: a base that is 8 but not 16 bytes
    aligned) and of the rollout storage's padded one, against the ctypes call on the same pointers; the row count
    grows and shrinks between the calls, so the cached workspace is replaced each time."""
    from lrl.ppo.rollout_storage import RolloutStorage
    c = case(R.NETS[0])
    total = 70
    obs, hist = c.obs[:total].contiguous(), c.hist[:total].contiguous()
    st = RolloutStorage(total, 1, [c.no], [R.NUM_PRIV], [c.nh], [NA], DEV)
    st.observation_histories[0].copy_(hist)
    padded = st.observation_histories[0]
    assert padded.stride(0) == hist_pad(c.nh)
    if hasattr(c.ac, "_student_ws"):
        del c.ac._student_ws
    for n_train in (37, 6, 5, 69):  # n = 33, 64, 65, 1
        n = total - n_train
        for h in (hist, padded):
            o, hv = obs[n_train:].contiguous(), h[n_train:]
            mean, lat = c.ac.act_student_fused(o, hv)
            torch.cuda.synchronize()
            # (the cache by its name: a workspace kept at an earlier, smaller size cannot be seen from outside)
            assert c.ac._student_ws[0] == n
            want = student(c, o, hv, hv.stride(0), n)
            same(npy(mean), want["mean"], f"n_train={n_train} pitch {hv.stride(0)}: mean")
            same(npy(lat), want["latent"], f"n_train={n_train} pitch {hv.stride(0)}: latent")


# ---- f. refusals -------------------------------------------------------------------------------------------------
def test_student_refusals():
    from lrl import _abi
    L = _abi.lib()
    c = case(R.NETS[0])
    n = 33
    assert L.lrl_ppo_act_student_workspace_bytes(C.byref(c.net), 0) < 0
    obs, hist = c.obs[:n].contiguous(), c.hist[:n].contiguous()
    ws, guard = workspace(L.lrl_ppo_act_student_workspace_bytes(C.byref(c.net), n))
    mean = torch.full((n, NA), NAN, device=DEV)
    lat = torch.full((n, c.net.latent), NAN, device=DEV)
    p = lambda t: t.data_ptr()
    for what, hist_ld, rows, mean_p, ws_p in (("hist_ld = num_hist - 1", c.nh - 1, n, p(mean), p(ws)),
                                              ("n = 0", c.nh, 0, p(mean), p(ws)),
                                              ("a null mean", c.nh, n, None, p(ws)),
                                              ("a null workspace", c.nh, n, p(mean), None)):
        rc = L.lrl_ppo_act_student(c.net, p(c.ac._flat), p(obs), p(hist), hist_ld, rows, mean_p, p(lat), ws_p,
                                   _abi.stream_of(DEV))
        torch.cuda.synchronize()
        msg = L.lrl_last_error()
        assert rc == INVALID, what
        assert msg and b"lrl_ppo_act_student" in msg, (what, msg)  # (the refusing call names itself)
        assert torch.isnan(mean).all() and torch.isnan(lat).all() and torch.isnan(ws).all(), what
    assert torch.isnan(guard).all()


# ---- g. teacher act against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n", NET_N)
def test_teacher_act_within_float64_bound(net, n, monkeypatch):
    c = case(net)
    rows = tuple(t[:n].contiguous() for t in (c.obs, c.priv, c.hist, c.eps))
    ref = first(c.teacher, n)
    t32 = torch_teacher(c, n) if c.name == "42x630" else None
    for fused in fused_settings(n):
        if fused is not None:
            monkeypatch.setenv("LRL_ACT_FUSED", fused)
        got = teacher(c, n, *rows)
        r = report(c, n, {None: "chain", "0": "chain", "1": "one-launch"}[fused], got, ref, R.TEACHER_OUT, t32)
        assert max(r.values()) <= 1, (fused, r)


@pytest.mark.parametrize("n", [33, 65])
def test_teacher_store_row_equals_outputs(n, monkeypatch):
    from lrl.ppo.rollout_storage import RolloutStorage
    c = case(R.NETS[0])
    rows = tuple(t[:n].contiguous() for t in (c.obs, c.priv, c.hist, c.eps))
    fields = ("observations", "privileged_observations", "observation_histories", "actions", "mu", "sigma", "values",
              "actions_log_prob")
    for fused in fused_settings(n):
        if fused is not None:
            monkeypatch.setenv("LRL_ACT_FUSED", fused)
        st = RolloutStorage(n, 3, [c.no], [R.NUM_PRIV], [c.nh], [NA], DEV)
        for f in fields:
            getattr(st, f).fill_(NAN)
        out = teacher(c, n, *rows, st=st, store_row=1)
        for f, k in (("mu", "mu"), ("actions", "actions"), ("values", "values"), ("actions_log_prob", "logp")):
            same(npy(getattr(st, f)[1]).reshape(out[k].shape), out[k], f"n={n} fused={fused}: storage {f}")
        same(npy(st.observation_histories[1]), npy(rows[2]), "storage history")
        for f in fields:
            assert torch.isnan(getattr(st, f)[0]).all() and torch.isnan(getattr(st, f)[2]).all(), f"{f}: other rows"
        assert max(R.ratios(out, first(c.teacher, n), R.TEACHER_OUT).values()) <= 1


# ---- h. trained weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 65, 257])
def test_trained_weights_within_bound(n, monkeypatch):
    """The checkpoint fixture's 64 rows cut to 63 and tiled to 65 and 257, on its trained weights."""
    c = case("trained")
    obs = c.obs[:n].contiguous()
    for form in (1, 3, 4):
        buf, view, ld = hist_form(form, c.hist[:n])
        r = report(c, n, form, student(c, obs, view, ld, n, buf=buf), first(c.student, n), R.STUDENT_OUT)
        assert max(r.values()) <= 1, (form, r)
    rows = tuple(t[:n].contiguous() for t in (c.obs, c.priv, c.hist, c.eps))
    for fused in fused_settings(n):
        if fused is not None:
            monkeypatch.setenv("LRL_ACT_FUSED", fused)
        r = report(c, n, {None: "chain", "0": "chain", "1": "one-launch"}[fused], teacher(c, n, *rows),
                   first(c.teacher, n), R.TEACHER_OUT)
        assert max(r.values()) <= 1, (fused, r)
