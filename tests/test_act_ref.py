"""tests/act_ref.py pinned on the CPU: the float64 restatement of the student and teacher acts agrees with the torch
modules in float64 and with the trained checkpoint's recorded outputs; its error bound is tight enough that the defects
it is there to catch move an output by more than ten bounds, and loose enough that a plain float32 evaluation of the
same formulas stays inside it on the very inputs the GPU tests feed (tests/test_act_rows_gpu.py)."""
import copy

import numpy as np
import pytest
import torch

import act_ref as R

N_ROWS = 257  # the GPU tests' largest row count: their rows are the first n of these


@pytest.mark.parametrize("no,nh", R.NETS)
def test_restatement_matches_torch_float64(no, nh):
    ac = R.make_net(no, nh)
    P = R.params_of(ac)
    ac64 = copy.deepcopy(ac).double()
    obs, priv, hist, eps = R.inputs(no, nh, 5)
    t = lambda a: torch.from_numpy(a).double()
    s, te = R.student_ref(P, obs, hist), R.teacher_ref(P, obs, priv, eps)
    with torch.no_grad():
        info = {}
        close = lambda a, b: np.testing.assert_allclose(a, b.numpy() if hasattr(b, "numpy") else b, rtol=1e-12)
        close(s["mean"], ac64.act_student(t(obs), t(hist), info))
        close(s["latent"], info["latents"])
        close(te["mu"], ac64.act_teacher(t(obs), t(priv)))
        close(te["values"], ac64.evaluate(t(obs), t(priv)))
        ac64.update_distribution(t(obs), t(priv))
        close(te["logp"], ac64.get_actions_log_prob(torch.from_numpy(te["actions"])))
        close(te["actions"], ac64.action_mean + ac64.std * t(eps))


def test_restatement_matches_trained_checkpoint():
    ac, g = R.trained_net()
    P = R.params_of(ac)
    s = R.student_ref(P, g["obs"], g["hist"])
    te = R.teacher_ref(P, g["obs"], g["priv"], np.zeros((64, 12)))
    for got, want in ((s["mean"], "mean_student"), (s["latent"], "latent_student"), (te["mu"], "mean_teacher"),
                      (te["values"], "value")):
        np.testing.assert_allclose(got, g[want], rtol=1e-5, atol=1e-5, err_msg=want)


def _both(P, obs, priv, hist, eps):
    return {**R.student_ref(P, obs, hist), **R.teacher_ref(P, obs, priv, eps)}


def _mutations(P, obs, priv, hist, eps):
    """{name: (outputs of the float64 reference with one defect, the outputs that defect corrupts)}: what a kernel
    with that defect would compute.  A defect is held to the outputs it would really move: one in the chain behind the
    latent must show in mean / mu / values, since the latent output is written in front of it."""
    S, T = R.STUDENT_OUT, R.TEACHER_OUT
    body = ("mean", "mu", "values")
    out = {}
    obs64, n = np.asarray(obs, np.float64), obs.shape[0]

    def params(**changed):
        Q = dict(P)
        Q.update({k.replace("__", "."): v for k, v in changed.items()})
        return Q

    def one_row(Q, r):
        """the unmutated outputs with row r from the parameters Q"""
        m, one = _both(P, obs, priv, hist, eps), _both(Q, obs[r:r + 1], priv[r:r + 1], hist[r:r + 1], eps[r:r + 1])
        for k in S + T:
            m[k] = m[k].copy()
            m[k][r] = one[k][0]
        return m

    def through_x(change):
        """mean / mu / values with X = change(obs, latent) in place of [obs | latent]"""
        m = {}
        for prefix, src, names in ((R.ADAPT, hist, ("mean",)), (R.ENCODER, priv, ("mu", "values"))):
            X = change(obs64, R.mlp(P, prefix, np.asarray(src, np.float64)))
            for k in names:
                m[k] = R.mlp(P, R.CRITIC if k == "values" else R.ACTOR, X)
        return m

    h = hist.copy()
    h[:, -1] = 0
    out["last history column dropped"] = _both(P, obs, priv, h, eps), S
    h = hist.copy()
    h[:, -16:] = 0
    out["history columns num_hist-16 onward dropped"] = _both(P, obs, priv, h, eps), S
    Q = params(actor_body__2__weight=P[R.CRITIC + ".2.weight"])
    out["critic's W2 in place of the actor's"] = _both(Q, obs, priv, hist, eps), ("mean", "mu")
    # one bias (the largest) of the last hidden layer dropped for one row: the actor body's 128-wide layer, and the
    # 32-wide one of the adaptation module
    for key, outs in ((R.ACTOR + ".4.bias", ("mean", "mu")), (R.ADAPT + ".2.bias", S)):
        bias = P[key].copy()
        bias[int(np.abs(bias).argmax())] = 0
        name = f"one bias of the last hidden layer dropped for one row ({key})"
        out[name] = one_row(params(**{key: bias}), n // 2), outs
    # the latent one column late in X: column num_obs stays zero, the last latent falls off X's end.  (The latent
    # output is a copy of the same columns the adaptation module wrote, so it does not show there.)
    out["latent one column late in X"] = through_x(
        lambda o, lat: np.concatenate([o, np.zeros((n, 1)), lat[:, :-1]], -1)), body
    out["std read reversed"] = _both(params(std=P["std"][::-1].copy()), obs, priv, hist, eps), ("actions", "logp")
    # and what the row classes of the GPU tests are there for, in the bodies behind the latent
    out["X's last float4 dropped from body 1 (k tail)"] = through_x(
        lambda o, lat: np.concatenate([o, lat[:, :-4], np.zeros((n, 4))], -1)), body
    out["the latent dropped from X"] = through_x(lambda o, lat: np.concatenate([o, 0 * lat], -1)), body
    W2 = P[R.ACTOR + ".2.weight"].copy()
    W2[:, -1] = 0
    Q = params(actor_body__2__weight=W2)
    out["the actor W2's last k column dropped"] = _both(Q, obs, priv, hist, eps), ("mean", "mu")
    Q = params(actor_body__6__bias=0 * P[R.ACTOR + ".6.bias"])
    out["the actor head's bias dropped"] = _both(Q, obs, priv, hist, eps), ("mean", "mu")
    return out


@pytest.mark.parametrize("no,nh", R.NETS)
def test_listed_defects_move_an_output_by_ten_bounds(no, nh):
    """Each defect, restated in float64, against the unmutated reference and its bound, on the GPU tests' inputs; a
    defect is held to the outputs it would really corrupt (a defect behind the latent to mean / mu / values, not to the
    latent output in front of it).  The test prints, per output, the bound relative to the value (medians: mean, mu and
    values 0.3 - 0.6 %, latent 0.08 - 0.2 %, actions 0.02 %, logp 7e-7) and every defect's worst element in bounds.
    The smallest of them, over the outputs named, for (42, 630) / (48, 720) / (235, 3525):
        last history column dropped (latent)                          425 / 536 / 83
        history columns num_hist-16 onward dropped (latent)          1320 / 1100 / 257
        critic's W2 in place of the actor's (mu)                     2620 / 2470 / 2530
        one bias dropped for one row, actor's last hidden layer (mu)   21 / 24 / 17     (student mean: 13 / 13 / 8)
        one bias dropped for one row, adaptation module (latent)       64 / 88 / 44
        latent one column late in X (mu)                              330 / 248 / 128   (mean 217 / 162 / 59)
        std read reversed (actions)                                   3e4 / 3e4 / 2e4   (logp: unmoved, z = eps)
        X's last float4 dropped from body 1 (mu)                      121 / 107 / 48    (mean 76 / 60 / 22)
        the latent dropped from X (mu)                                209 / 176 / 83
        the actor W2's last k column dropped (mu)                     182 / 156 / 151
        the actor head's bias dropped (mu)                            434 / 433 / 326
    With injected noise logp does not depend on mu (the kernel scores actions - mu, which is std * eps): it checks the
    head alone."""
    P = R.params_of(R.make_net(no, nh))
    obs, priv, hist, eps = R.inputs(no, nh, N_ROWS)
    base = _both(P, obs, priv, hist, eps)
    for k in R.STUDENT_OUT + R.TEACHER_OUT:
        b, v = np.median(base["bound_" + k]), np.median(np.abs(base[k]))
        print(f"act_ref bound net=({no},{nh}) {k}: median bound {b:.2e}, median |value| {v:.2e}, ratio {b / v:.1e}")
    for name, (mut, outs) in _mutations(P, obs, priv, hist, eps).items():
        r = R.ratios(mut, base, outs)
        print(f"act_ref sensitivity net=({no},{nh}) {name}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
        assert max(r.values()) > 10, (name, r)


@pytest.mark.parametrize("net", R.NETS + ("trained",))
def test_float32_evaluation_stays_inside_the_bound(net):
    """The same formulas in numpy float32 against the float64 reference, on the GPU tests' own inputs (every net's 257
    rows; the checkpoint's rows tiled to 257): every element within its bound.  Worst error / bound on the CPU this
    was written on: logp 0.32 / 0.25 / 0.27 for the three nets and 0.12 for the trained one (the cancellation in
    actions - mu, which dz bounds at its worst case); mean, latent, mu, actions and values 4e-3 at the most (1e-3 on
    the trained net): a worst case over every rounding against roundings that add like a random walk, under the
    1e-6 product bar that the fp32 kernels themselves meet five times over."""
    if net == "trained":
        ac, g = R.trained_net()
        obs, priv, hist, eps = R.trained_rows(g, N_ROWS)
    else:
        ac = R.make_net(*net)
        obs, priv, hist, eps = R.inputs(*net, N_ROWS)
    P = R.params_of(ac)
    rs = R.ratios(R.student_eval(P, obs, hist), R.student_ref(P, obs, hist), R.STUDENT_OUT)
    rt = R.ratios(R.teacher_eval(P, obs, priv, eps), R.teacher_ref(P, obs, priv, eps), R.TEACHER_OUT)
    print(f"act_ref float32 slack net={net}: " + " ".join(f"{k}={v:.2e}" for k, v in {**rs, **rt}.items()))
    assert max(rs.values()) < 1 and max(rt.values()) < 1, (rs, rt)
