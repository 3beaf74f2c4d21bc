"""The depth encoder's native path (csrc/lrl_vision.hip through lrl.vision) on the GPU against the fp64 restatement
(tests/vision_ref.py), and the distiller on a rough-terrain Go1 env.

Accuracy bar.  Per tensor (features, output, loss, every gradient field): err = max|x - fp64| / max|fp64|, measured
for the native path (err_native) and for torch's fp32 CPU form on the same inputs (err_torch32); the bar is
err_native <= K * err_torch32 + FLOOR.  K is twice the worst err_native / err_torch32 ratio measured on an MI355X over
this file's cases, and not below 2 (the margin the project's epilogue tests give a different summation order); the
measured ratios stand beside the constant.  FLOOR = 2^-22 (four fp32 roundings at the scale of the tensor's largest
entry) is there for the tensors on which torch's own error happens to be next to nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import depth_scenes as ds
import vision_ref as vr
from lrl import _abi
from lrl import config as lcfg
from lrl import vision

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = vision.MAX_WORKGROUPS
# Measured on an MI355X over this file's cases (120 tensors; python -m pytest -s prints each): the worst ratios are
# 1.93 (fc1.bias's movement over the three Adam steps), 1.73 and 1.62 (fc2.weight and fc2.bias gradients, 48 x 64,
# batch 3), 1.41 (fc2.bias, 16 x 16, batch 513), 1.34 (fc1.weight, 16 x 16, batch 1027); the conv stack's own tensors
# (features, conv gradients) stay at or below 1.22.  K = 2 * 1.93, rounded up.
K = 3.9
FLOOR = 2.0 ** -22
SENT = 12345.678  # what every buffer holds before a call: a float no result takes
G = 256           # guard floats on each side of a buffer


def _guarded(n, dtype=torch.float32):
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device=DEV)
    return buf, buf[G:G + n]


def _intact(buf, n):
    return bool((buf[:G] == buf.new_tensor(SENT)).all() and (buf[G + n:] == buf.new_tensor(SENT)).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _encoder(h, w, extra, out, hidden, seed):
    torch.manual_seed(seed)
    enc = vision.DepthEncoder(h, w, out, extra_dim=extra, hidden=hidden, far=3.0)
    with torch.no_grad():  # biases of the size of the weights' effect, so a dropped or misplaced bias shows
        for k, p in enc.named_parameters():
            if k.endswith("bias"):
                p.uniform_(-0.3, 0.3)
    return enc


def _data(n, h, w, extra, out, seed):
    """images in [0, 3) m, extra rows at pitch extra + 3, target rows at pitch out + 2 (the padding holds junk)"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(n, h, w, generator=g) * 3.0
    ex = torch.randn(n, extra + 3, generator=g)
    tg = torch.randn(n, out + 2, generator=g)
    return img, ex, tg


def _forward(enc, img, ex, rows, batch):
    """lrl_vision_forward into guarded buffers: (out [batch, out], features [batch, F])"""
    L, net = vision.lib(), enc.net()
    obuf, out = _guarded(batch * enc.out_dim)
    fbuf, feat = _guarded(batch * enc.features)
    wfl = L.lrl_vision_workspace_bytes(C.addressof(net), batch) // 4
    wbuf, ws = _guarded(wfl)
    _abi.check(L.lrl_vision_forward(C.addressof(net), _p(enc.flat), _p(img), _p(ex) if enc.extra_dim else None,
                                    ex.stride(0) if enc.extra_dim else 0, _p(rows), batch, _p(out), _p(feat), _p(ws),
                                    _abi.stream_of(DEV)))
    torch.cuda.synchronize()
    assert _intact(obuf, out.numel()) and _intact(fbuf, feat.numel()) and _intact(wbuf, wfl)
    return out.view(batch, -1).clone(), feat.view(batch, -1).clone()


def _forward_backward(enc, img, ex, tg, rows, batch):
    """lrl_vision_forward_backward into guarded buffers: (loss, grads flat); checks what the call must leave alone"""
    L, net = vision.lib(), enc.net()
    total = enc.flat.numel()
    gbuf, grads = _guarded(total)
    lbuf, loss = _guarded(1, torch.float64)
    wfl = L.lrl_vision_workspace_bytes(C.addressof(net), batch) // 4
    wbuf, ws = _guarded(wfl)
    _abi.check(L.lrl_vision_forward_backward(
        C.addressof(net), _p(enc.flat), _p(grads), _p(img), _p(ex) if enc.extra_dim else None,
        ex.stride(0) if enc.extra_dim else 0, _p(tg), tg.stride(0), _p(rows), batch, _p(loss), _p(ws),
        _abi.stream_of(DEV)))
    torch.cuda.synchronize()
    assert _intact(gbuf, total) and _intact(lbuf, 1) and _intact(wbuf, wfl)
    # grads: every field written, the padding between fields left alone
    written = torch.zeros(total, dtype=torch.bool, device=DEV)
    for k, (off, shape) in enc.offsets.items():
        written[off:off + int(np.prod(shape))] = True
    sent = grads == grads.new_tensor(SENT)
    assert not sent[written].any() and sent[~written].all()
    # the conv gradients' partial rows: one per workgroup, the tail of each row untouched
    off, nrows, pitch, used = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    _abi.check(L.lrl_debug_vision_partials(C.addressof(net), batch, C.byref(off), C.byref(nrows), C.byref(pitch),
                                           C.byref(used)))
    assert nrows.value == min(batch, CAP) and used.value == 14304 and pitch.value > used.value
    part = ws[off.value:off.value + nrows.value * pitch.value].view(nrows.value, pitch.value)
    assert (part[:, used.value:] == part.new_tensor(SENT)).all() and not (part[:, :used.value] == SENT).any()
    return loss.clone()[0], grads.clone()


def _err(x, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


RATIOS = []


def _judge(case, name, native, torch32, ref):
    en, et = _err(native, ref), _err(torch32, ref)
    RATIOS.append((case, name, en, et))
    print(f"RATIO {case} {name}: err_native {en:.3e} err_torch32 {et:.3e} ratio {en / max(et, 1e-300):.2f} "
          f"bar {K * et + FLOOR:.3e}")
    return en <= K * et + FLOOR, f"{case} {name}: err_native {en:.3e} > {K} * {et:.3e} + {FLOOR:.3e}"


# (H, W, batch, E, out, hidden): every size at batch 1 and 3, E in {0, 5}, out in {1, 18, 187}, hidden in {16, 128};
# at 16 x 16 also the two batches beyond the grid cap (the image loop: one extra image, and two rounds plus three)
CASES = [(16, 16, 1, 0, 1, 16), (16, 16, 3, 5, 18, 128), (16, 24, 1, 5, 187, 16), (16, 24, 3, 0, 18, 128),
         (48, 64, 1, 5, 187, 128), (48, 64, 3, 0, 1, 16), (48, 64, 3, 5, 18, 128), (16, 16, CAP + 1, 5, 18, 16),
         (16, 16, 2 * CAP + 3, 0, 187, 128)]


@pytest.mark.parametrize("h, w, batch, extra, out, hidden", CASES)
def test_native_forward_and_gradients_against_fp64(h, w, batch, extra, out, hidden):
    case = f"{h}x{w} b{batch} E{extra} out{out} hid{hidden}"
    enc = _encoder(h, w, extra, out, hidden, seed=h + w + batch)
    img, ex, tg = _data(batch, h, w, extra, out, seed=batch + extra)
    # fp64 restatement and torch's fp32 CPU form, on the fp32 values the device gets
    P = {k: v.detach().double().numpy() for k, v in enc.state_dict().items()}
    exu, tgu = ex[:, :extra], tg[:, :out]
    rl, rg, r = vr.mse_grads(P, img.numpy(), exu.numpy() if extra else None, tgu.numpy(), float(np.float32(enc.input_scale)))
    enc.zero_grad()
    t_feat = enc.conv_features(img).detach()
    t_pred = enc(img, exu)
    t_loss = F.mse_loss(t_pred, tgu)
    t_loss.backward()
    t_grads = {k: p.grad.clone() for k, p in enc.named_parameters()}
    # the native path
    enc = enc.to(DEV)
    dimg, dex, dtg = img.to(DEV), ex.to(DEV), tg.to(DEV)
    n_out, n_feat = _forward(enc, dimg, dex, None, batch)
    n_loss, n_grads = _forward_backward(enc, dimg, dex, dtg, None, batch)
    # determinism: a second call gives the same bits
    o2, f2 = _forward(enc, dimg, dex, None, batch)
    l2, g2 = _forward_backward(enc, dimg, dex, dtg, None, batch)
    assert torch.equal(o2, n_out) and torch.equal(f2, n_feat) and torch.equal(l2, n_loss) and torch.equal(g2, n_grads)
    # the module's own entry points are the same calls
    assert torch.equal(enc.forward_native(dimg, dex), n_out)
    assert torch.equal(enc.mse_backward_native(dimg, dex, dtg), n_loss)
    assert torch.equal(enc.flat_grad, n_grads.masked_fill(n_grads == SENT, 0.0))
    fails = []
    checks = [("features", n_feat.cpu().numpy(), t_feat.numpy(), r["features"]),
              ("output", n_out.cpu().numpy(), t_pred.detach().numpy(), r["pred"]),
              ("loss", n_loss.item(), t_loss.item(), rl)]
    for k, (off, shape) in enc.offsets.items():
        checks.append((k, n_grads[off:off + int(np.prod(shape))].view(shape).cpu().numpy(), t_grads[k].numpy(), rg[k]))
    for name, nat, t32, ref in checks:
        ok, msg = _judge(case, name, nat, t32, ref)
        if not ok:
            fails.append(msg)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("h, w, extra", [(16, 24, 5), (48, 64, 0)])
def test_rows_gather_equals_gathered_copies_and_rows_are_independent(h, w, extra):
    out, hidden, n = 18, 16, 7
    enc = _encoder(h, w, extra, out, hidden, seed=5).to(DEV)
    img, ex, tg = (t.to(DEV) for t in _data(n, h, w, extra, out, seed=9))
    rows = torch.tensor([5, 2, 2, 6, 0, 5], device=DEV)  # repeats, out of order, not every row
    b = rows.numel()
    go, gf = _forward(enc, img, ex, rows, b)
    gl, gg = _forward_backward(enc, img, ex, tg, rows, b)
    co, cf = _forward(enc, img[rows].contiguous(), ex[rows].contiguous(), None, b)
    cl, cg = _forward_backward(enc, img[rows].contiguous(), ex[rows].contiguous(), tg[rows].contiguous(), None, b)
    assert torch.equal(go, co) and torch.equal(gf, cf) and torch.equal(gl, cl) and torch.equal(gg, cg)
    assert torch.equal(gf[1], gf[2]) and torch.equal(gf[0], gf[5]) and not torch.equal(gf[0], gf[1])
    # a feature row is the same bits alone (batch 1) and inside a batch of 3
    three = torch.tensor([4, 2, 1], device=DEV)
    _, f3 = _forward(enc, img, ex, three, 3)
    for i, row in enumerate(three.tolist()):
        _, f1 = _forward(enc, img, ex, torch.tensor([row], device=DEV), 1)
        assert torch.equal(f1[0], f3[i])
    _, fall = _forward(enc, img, ex, None, n)
    assert torch.equal(fall[three], f3)


def test_native_calls_refuse_bad_arguments():
    enc = _encoder(16, 16, 5, 18, 16, seed=1).to(DEV)
    img, ex, tg = (t.to(DEV) for t in _data(2, 16, 16, 5, 18, seed=1))
    L, net = vision.lib(), enc.net()
    ws = torch.empty(L.lrl_vision_workspace_bytes(C.addressof(net), 2), dtype=torch.uint8, device=DEV)
    out = torch.empty(2, 18, device=DEV)
    blank = vision.LrlVisionNet()  # (never handed to lrl_vision_net_init)
    args = lambda **kw: [kw.get("net", C.addressof(net)), _p(enc.flat), _p(img), kw.get("ex", _p(ex)), kw.get("ld", 8),
                         None, kw.get("batch", 2), _p(out), None, _p(ws), None]
    for kw, word in (({"batch": 0}, "batch"), ({"ex": None}, "extra"), ({"ld": 4}, "ld_extra"),
                     ({"net": C.addressof(blank)}, "lrl_vision_net_init")):
        assert L.lrl_vision_forward(*args(**kw)) == -1
        assert word in L.lrl_last_error().decode()
    with pytest.raises(ValueError, match="contiguous float32"):
        enc.forward_native(img[:, :, :8], ex)
    with pytest.raises(ValueError, match="int64"):
        enc.forward_native(img, ex, rows=torch.zeros(2, dtype=torch.int32, device=DEV))


# ---- the distiller on a rough-terrain Go1 env ----
STEPS, INTERVAL, ENVS = 10, 5, 64


def _rough_env(seed=11):
    from lrl.env import LeggedRobotEnv
    cfg = ds.go1_trimesh_cfg(ENVS)
    cfg.terrain.measure_heights = True
    npts = len(cfg.terrain.measured_points_x) * len(cfg.terrain.measured_points_y)
    cfg.env.num_observations = 42 + npts
    lcfg.add_depth_camera(cfg, update_interval=INTERVAL)
    env = LeggedRobotEnv(DEV, cfg=cfg, seed=seed)
    assert not env.depth_refreshed  # no step yet
    env.reset()  # (reset all, then one zero-action step: the sensor's first tick, a full refresh)
    assert env.depth_refreshed
    return env, npts


def _rollout(env, distiller):
    """STEPS steps under fixed actions; with a distiller: collect at the refresh steps, train and predict in between.
    Returns what the env produced."""
    g = torch.Generator().manual_seed(3)
    trace, fed = [], []
    for step in range(STEPS):
        act = (torch.rand(ENVS, 12, generator=g) - 0.5).to(DEV)
        obs, rew, done, _ = env.step(act)
        if distiller is not None:
            if env.depth_refreshed:
                distiller.collect(obs)
                fed.append((step, env.depth_images.clone(), obs.clone()))
            if distiller.size:
                distiller.update(1)
                distiller.predict_obs(obs)
        trace.append((obs.clone(), rew.clone(), done.clone(), env.depth_images.clone(), env.root_states.clone(),
                      env.dof_pos.clone()))
    return trace, fed


@pytest.fixture(scope="module")
def distilled():
    env, npts = _rough_env()
    try:
        enc = _encoder(48, 64, 42, npts, 128, seed=2).to(DEV)
        d = vision.DepthDistiller(env, enc, capacity=256, batch_size=64, lr=1e-3)
        assert d.native
        trace, fed = _rollout(env, d)
    finally:
        env.close()
    return d, trace, fed, npts


def test_distiller_collects_the_refresh_steps(distilled):
    d, trace, fed, npts = distilled
    assert npts == 187 and (d.first, d.num_scan) == (42, 187)
    assert [s for s, _, _ in fed] == [4, 9]  # the sensor's ticks 5 and 10 (reset's own step was tick 0): every fifth
    assert d.size == 2 * ENVS == 128 and d.head == 128
    for i, (_, img, obs) in enumerate(fed):
        assert torch.equal(d.images[i * ENVS:(i + 1) * ENVS], img)
        assert torch.equal(d.extra[i * ENVS:(i + 1) * ENVS], obs[:, :42])
        assert torch.equal(d.target[i * ENVS:(i + 1) * ENVS], obs[:, 42:])
    assert float(d.images[:128].min()) >= 0.05 and float(d.images[:128].max()) <= 3.0
    assert float(d.images[:128].std()) > 0.05 and float(d.target[:128].std()) > 0  # a scene, and a scan to regress


def test_rollout_with_a_distiller_is_bit_identical_to_one_without(distilled):
    _, trace, _, _ = distilled
    env, _ = _rough_env()
    try:
        bare, _ = _rollout(env, None)
    finally:
        env.close()
    for step, (a, b) in enumerate(zip(trace, bare)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), step


def _twin(d, state, dtype, native, dev=DEV):
    """A distiller on a copy of d's rings (on `dev`, as `dtype`) whose encoder starts from `state`, with fresh Adam
    state; it never steps an env."""
    import types
    enc = vision.DepthEncoder(48, 64, d.num_scan, extra_dim=d.first, hidden=128, far=3.0)
    enc.load_state_dict(state)
    enc = enc.to(dev).to(dtype)
    env = types.SimpleNamespace(cfg=d.env.cfg, depth_images=d.env.depth_images.to(dev))
    t = vision.DepthDistiller(env, enc, capacity=d.capacity, batch_size=64, lr=1e-3, native=native)
    t.images, t.obs = d.images.to(dev, dtype), d.obs.to(dev, dtype)
    t.extra, t.target = t.obs[:, :t.first], t.obs[:, t.first:]
    t.size, t.head = d.size, d.head
    return t


def test_three_updates_native_and_torch_agree(distilled):
    d, _, _, _ = distilled
    start = {k: v.clone() for k, v in _encoder(48, 64, 42, 187, 128, seed=4).state_dict().items()}
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(d.size, (64,), generator=g) for _ in range(3)]
    runs = {}
    # the native path on the GPU; the torch form on the CPU in fp32 (err_torch32) and in fp64 (the reference)
    for name, dtype, native, dev in (("native", torch.float32, True, DEV), ("torch32", torch.float32, False, "cpu"),
                                     ("fp64", torch.float64, False, "cpu")):
        t = _twin(d, start, dtype, native, dev)
        assert t.native == native
        losses = [t.update(1, rows=[r.to(dev)]).item() for r in rows]
        runs[name] = (losses, {k: v.detach().double().cpu().numpy() for k, v in t.encoder.state_dict().items()})
    fails = []
    ok, msg = _judge("3 updates", "losses", runs["native"][0], runs["torch32"][0], runs["fp64"][0])
    if not ok:
        fails.append(msg)
    for k in vr.KEYS:  # the parameters' movement over the three steps
        p0 = start[k].double().numpy()
        ok, msg = _judge("3 updates", "delta " + k, runs["native"][1][k] - p0, runs["torch32"][1][k] - p0,
                         runs["fp64"][1][k] - p0)
        if not ok:
            fails.append(msg)
    assert not fails, "\n".join(fails)


def test_thirty_adam_steps_on_one_batch_lower_the_loss(distilled):
    d, _, _, _ = distilled
    t = _twin(d, _encoder(48, 64, 42, 187, 128, seed=6).state_dict(), torch.float32, True)
    rows = torch.arange(64, device=DEV) * 2
    first = t.update(1, rows=[rows])
    t.update(28, rows=[rows] * 28)
    last = t.update(1, rows=[rows])
    print(f"loss on one batch of 64: {first.item():.5f} -> {last.item():.5f} after 30 Adam steps")
    assert last.item() < first.item()
