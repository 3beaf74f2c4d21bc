"""Bit-identity check of a change to the PPO host path (csrc/lrl_ppo.hip): one call each of lrl_ppo_act (with a rollout
store), lrl_ppo_act_student, lrl_ppo_forward_backward + lrl_ppo_optimizer_step and lrl_ppo_adaptation_forward_backward +
lrl_ppo_adaptation_step under the library LRL_LIB names, for the blind (42-obs), perceptive (235-obs) and plain
(lrl.hlp, 14 -> 3; no student / adaptation calls) nets at 37 and 256 rows, fixed seeds, injected eps.  Every output, the
storage rows the act wrote, the gradient / parameter / moment buffers, ctrl and the workspaces (pre-filled with a
sentinel, so bytes no kernel writes compare too) are saved; `compare` diffs two such files.  With LRL_GEMM_TRACE=1 the
library logs every product to stderr: two runs' logs must be identical line for line.
usage: LRL_LIB=... LRL_GEMM_TRACE=1 python scripts/ab_ppo_calls.py run <out.npz> 2> <trace.log>
       python scripts/ab_ppo_calls.py compare <a.npz> <b.npz>"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

SENT = 0x7FA5A5A5  # a NaN with a payload no kernel produces
NETS = {"blind": ("ppo", 42, 18, 630, 12), "perceptive": ("ppo", 235, 18, 3525, 12), "plain": ("hlp", 14, 18, 16, 3)}
ROWS = (37, 256)
T = 4


def _calls(tag, kind, no, npriv, nh, na, n, out):
    import torch
    from lrl import _abi
    if kind == "hlp":
        from lrl.hlp import PPO, ActorCritic
    else:
        from lrl.ppo.actor_critic import ActorCritic
        from lrl.ppo.ppo import PPO
    dev = "cuda:0"
    L = _abi.lib()
    torch.manual_seed(0)
    ac = ActorCritic(no, npriv, nh, na).cuda()
    alg = PPO(ac, device=dev, fused=True)
    alg.init_storage(n, T, [no], [npriv], [nh], [na])
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    s = alg.storage
    with torch.no_grad():
        for name in ("observations", "privileged_observations", "observation_histories", "actions", "mu", "values"):
            getattr(s, name).copy_(rn(*getattr(s, name).shape))
        s.sigma.fill_(1.0)
        s.returns.copy_(s.values + 0.3 * rn(*s.values.shape))
        a = rn(*s.advantages.shape)
        s.advantages.copy_((a - a.mean()) / a.std())
        s.actions_log_prob.copy_((-11.0 if na == 12 else -4.3) + rn(*s.values.shape))
    net = ac.flatten_parameters()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = _abi.stream_of(torch.device(dev))
    put = lambda k, t: out.__setitem__(f"{tag}/{k}", t.detach().cpu().numpy().copy())

    def sentinel_ws(nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return torch.full((nbytes // 4,), SENT, dtype=torch.int32, device=dev)

    # ---- rollout act into storage row 1 ----
    obs, priv, hist, eps = rn(n, no), rn(n, npriv), rn(n, nh), rn(n, na)
    ac._act_ws = (n, sentinel_ws(L.lrl_ppo_act_workspace_bytes(C.byref(net), C.c_int32(n))))
    res = ac.act_fused(obs, priv, hist=hist, eps=eps, store=s.store_desc(), store_row=1)
    for k, t in zip(("actions", "mu", "values", "logp"), res):
        put("act_" + k, t)
    put("act_ws", ac._act_ws[1])
    for name in ("observations", "privileged_observations", "observation_histories", "actions", "values",
                 "actions_log_prob", "mu", "sigma"):
        put("store_" + name, getattr(s, name)[1])
    # ---- student act ----
    if not net.plain:
        ac._student_ws = (n, sentinel_ws(L.lrl_ppo_act_student_workspace_bytes(C.byref(net), C.c_int32(n))))
        mean, latent = ac.act_student_fused(obs, s.observation_histories[0])
        put("student_mean", mean)
        put("student_latent", latent)
        put("student_ws", ac._student_ws[1])
    # ---- one minibatch: forward / backward + optimiser step, adaptation forward / backward + step ----
    mb = n * T // 4
    st = alg._native_state(mb)
    hp, grads, ctrl, m, v = st["hp"], st["grads"], st["ctrl"], st["exp_avg"], st["exp_avg_sq"]
    ws = st["ws"] = sentinel_ws(st["ws"].numel())
    ctrl[0] = 1e-3
    rows = torch.randperm(n * T, device=dev, generator=torch.Generator(device=dev).manual_seed(7))[:mb].contiguous()
    fl = lambda t: t.flatten(0, 1)
    batch = _abi.LrlPpoBatch()
    for k, t in dict(obs=s.observations, priv=s.privileged_observations, hist=s.observation_histories, actions=s.actions,
                     values=s.values, returns=s.returns, logp=s.actions_log_prob, adv=s.advantages, mu=s.mu,
                     sigma=s.sigma).items():
        setattr(batch, k, fl(t).data_ptr())
    batch.rows, batch.batch, batch.hist_ld = rows.data_ptr(), mb, fl(s.observation_histories).stride(0)
    params = ac._flat
    _abi.check(L.lrl_ppo_forward_backward(C.byref(net), ptr(params), ptr(grads), C.byref(batch), C.byref(hp), ptr(ws),
                                          ptr(ctrl), stream))
    torch.cuda.synchronize()
    put("update_grads", grads)
    put("update_ws", ws)
    put("update_ctrl", ctrl)
    _abi.check(L.lrl_ppo_optimizer_step(C.byref(net), ptr(params), ptr(grads), ptr(m), ptr(v), C.c_int64(1),
                                        C.c_float(1.0), C.byref(hp), ptr(ws), ptr(ctrl), stream))
    torch.cuda.synchronize()
    for k, t in dict(step_params=params, step_exp_avg=m, step_exp_avg_sq=v, step_ctrl=ctrl).items():
        put(k, t)
    if not net.plain:
        ws.fill_(SENT)
        _abi.check(L.lrl_ppo_adaptation_forward_backward(C.byref(net), ptr(params), None, ptr(grads), C.byref(batch),
                                                         ptr(ws), ptr(ctrl), stream))
        torch.cuda.synchronize()
        put("adapt_grads", grads)
        put("adapt_ws", ws)
        put("adapt_ctrl", ctrl)
        _abi.check(L.lrl_ppo_adaptation_step(C.byref(net), ptr(params), ptr(grads), ptr(m), ptr(v), C.c_int64(1),
                                             C.c_double(1e-3), C.c_float(1.0), C.byref(hp), ptr(ctrl), stream))
        torch.cuda.synchronize()
        for k, t in dict(astep_params=params, astep_exp_avg=m, astep_exp_avg_sq=v, astep_ctrl=ctrl).items():
            put(k, t)


def run(path):
    out = {}
    for name, spec in NETS.items():
        for n in ROWS:
            _calls(f"{name}{n}", *spec, n, out)
    for k, x in out.items():  # the calls computed something: no output or updated buffer holds a NaN / inf
        if not k.endswith(("_ws", "_ctrl")) and x.dtype.kind == "f":
            assert np.isfinite(x).all() and np.abs(x).sum() > 0, k
    np.savez(path, **out)
    print("saved", path, len(out), "arrays")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"{k}: only in one file")
    differing = 0
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        nd = 0 if same else (int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape else -1)
        if not same:
            print(f"{k}: DIFFERS ({nd} bytes of {x.nbytes})")
            differing += 1
    total = len(set(A.files) & set(B.files))
    print(f"{total - differing} of {total} arrays bit-identical" + ("" if differing or bad else ": IDENTICAL"))
    return differing + len(bad)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
