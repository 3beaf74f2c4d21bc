"""The depth sensor model on cuda:0 (lrl_sim_depth_sense, and LeggedRobotEnv with the Cfg.depth_sensor group) against
the numpy restatement tests/depth_sensor_ref.py, which tests/test_depth_sensor_ref.py pins on hand cases.

Judged exactly: head, latency, which pixels are far / lost, every delivered frame against the kernel's own ring, every
array of an env a call must not touch, and, with the noise off, every value (bit-equal to the float32 restatement).
Judged within depth_sensor_ref.value_bar (aux_ref.policy_noise_bound scaled by sigma, plus the roundings of sigma
itself): the values of kept pixels with the noise on and the quantisation off.  With both on, a pixel whose reference
value before quantisation lies within that bar of a half-step may land one step off; such pixels stay under 1 % of an
image (tests/test_depth_sensor_ref.py: the reference alone has about 5e-4 of them).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import depth_scenes as ds
import depth_sensor_ref as sr
import draws_cases as dc
import helpers as hp
from lrl import _abi
from lrl import config as lcfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
N = 5
FAR = 3.0
SIZES = [(13, 17), (30, 40)]  # (H, W): 221 pixels, one partial pass; 1200 pixels, four full passes and a 176-pixel tail
# (mode, flagged envs, frame): fill-all, push, push with env 3 flagged, reset-only with env 1 flagged, reset-only with
# none flagged (nothing written), then pushes; one frame has its high word set
# (the fill at frame 2 draws the delays 0, 1, 0, 2, 0: pushes at every delay of [0, 2] follow)
CALLS = [(sr.FILL, (), 2), (sr.PUSH, (), 3), (sr.PUSH, (3,), 4), (sr.RESET_ONLY, (1,), 5), (sr.RESET_ONLY, (), 6),
         (sr.PUSH, (), dc.WRAP), (sr.PUSH, (), dc.WRAP + 1), (sr.PUSH, (), 11)]
NOISE = dict(noise_a=0.002, noise_b=0.01)
KEYS = ("ring", "head", "latency", "sensed")


def _struct(p):
    s = _abi.LrlDepthSensor()
    for f, _ in _abi.LrlDepthSensor._fields_:
        setattr(s, f, getattr(p, f))
    return s


def _alloc(n, p, fill=-7.0):
    D = p.latency_max + 1
    return dict(ring=torch.full((n, D, p.height, p.width), fill, device=DEV),
                head=torch.full((n,), int(fill), dtype=torch.int32, device=DEV),
                latency=torch.full((n,), int(fill), dtype=torch.int32, device=DEV),
                sensed=torch.full((n, p.height, p.width), fill, device=DEV))


def _np(st):
    return {k: hp.npy(st[k]).copy() for k in KEYS}


def _sense(sim, p, mode, frame, depth, st, first=0, count=N, uniforms=None, row=0):
    """lrl_sim_depth_sense on envs [first, first + count), the arrays starting at their row ``row``; returns rc."""
    rc = sim.L.lrl_sim_depth_sense(sim.h, C.byref(_struct(p)), first, count, mode, C.c_uint64(frame),
                                   hp.vp(depth[row:]), None if uniforms is None else hp.vp(uniforms[row:]),
                                   hp.vp(st["ring"][row:]), hp.vp(st["head"][row:]), hp.vp(st["latency"][row:]),
                                   hp.vp(st["sensed"][row:]), hp.stream())
    hp.sync()
    return rc


def _flags(sim, envs):
    f = np.zeros(N, np.uint8)
    f[list(envs)] = 1
    sim.t(_abi.T_RESET)[:N].copy_(hp.dev(f, torch.uint8))
    return f


def _exact(k, h, w):
    """The exact images of call k: tests/depth_sensor_ref.scene, moved a little every call, its far patch kept."""
    z = sr.scene(N, h, w, FAR)
    return np.where(z >= F32(FAR), F32(FAR), z + F32(0.013 * k)).astype(F32)


@pytest.fixture(scope="module")
def sim():
    with hp.mc_sim(N, offset=dc.BIG_OFFSET, seed=dc.SEED) as s:
        saved = s.t(_abi.T_RESET).clone()
        yield s
        s.t(_abi.T_RESET).copy_(saved)


@functools.lru_cache(None)
def _reference(h, w, dtype, **kw):
    """The reference's states and per-call sensed frames over CALLS (computed once per parameter set)."""
    p = sr.params(w, h, far=FAR, latency=(0, 2), invalid_value=-1.0, **kw)
    st = sr.state(N, p, dtype=dtype)
    out = []
    for k, (mode, envs, frame) in enumerate(CALLS):
        f = np.zeros(N, np.uint8)
        f[list(envs)] = 1
        v = sr.call(st, p, dc.BIG_OFFSET, dc.SEED, mode, f, frame, _exact(k, h, w), dtype=dtype)
        out.append((v, {k_: a.copy() for k_, a in st.items()}))
    return p, out


def _run(sim, p, h, w):
    """CALLS on the GPU from freshly poisoned arrays: the state after every call."""
    st = _alloc(N, p)
    out = []
    for k, (mode, envs, frame) in enumerate(CALLS):
        _flags(sim, envs)
        assert _sense(sim, p, mode, frame, hp.dev(_exact(k, h, w)), st) == 0, sim.L.lrl_last_error()
        out.append(_np(st))
    return out


def _touched(mode, envs):
    return [b for b in range(N) if mode != sr.RESET_ONLY or b in envs]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("which", ["edge and dropout", "edge only", "dropout only"])
def test_noise_off_is_bit_equal_to_the_float32_restatement(sim, h, w, which):
    kw = dict(quant=0.01, edge_thresh=0.0 if which == "dropout only" else 0.1,
              dropout_p=0.0 if which == "edge only" else 0.05)
    p, ref = _reference(h, w, F32, **kw)
    got = _run(sim, p, h, w)
    lost = far = 0
    for k, (g, (v, r)) in enumerate(zip(got, ref)):
        for key in KEYS:
            hp.same(g[key], r[key], f"{which} {h}x{w} call {k} {key}")
        lost += int((v == F32(-1.0)).sum())
        far += int((v == F32(FAR)).sum())
    assert lost > 0 and far > 0  # the masks were not empty
    # call 4 (reset-only, no flag set) wrote nothing; call 3 wrote env 1 alone
    for key in KEYS:
        hp.same(got[4][key], got[3][key], key)
        hp.same(np.delete(got[3][key], 1, 0), np.delete(got[2][key], 1, 0), key)
    assert got[3]["head"][1] == 0 and got[2]["head"][3] == 0 and got[2]["head"][0] == 2


@pytest.mark.parametrize("h,w", SIZES)
def test_noise_on_values_within_the_bar_and_the_ring_delivers(sim, h, w):
    kw = dict(edge_thresh=0.1, dropout_p=0.02, **NOISE)
    p, ref = _reference(h, w, np.float64, **kw)
    got = _run(sim, p, h, w)
    D = p.latency_max + 1
    worst, kept = 0.0, 0
    prev = None
    for k, ((mode, envs, frame), g, (v64, r)) in enumerate(zip(CALLS, got, ref)):
        np.testing.assert_array_equal(g["head"], r["head"], str(k))
        np.testing.assert_array_equal(g["latency"], r["latency"], str(k))
        z = _exact(k, h, w)
        for b in range(N):
            if b not in _touched(mode, envs):
                for key in KEYS:
                    hp.same(g[key][b], prev[key][b], f"call {k} env {b} {key} (untouched)")
                continue
            hd, lat = int(g["head"][b]), int(g["latency"][b])
            v = g["ring"][b, hd]  # the frame this call sensed
            hp.same(g["sensed"][b], g["ring"][b, (hd - lat + D) % D], f"call {k} env {b}: delivered frame")
            if mode != sr.PUSH or b in envs:
                for d in range(D):
                    hp.same(g["ring"][b, d], v, f"call {k} env {b}: a fill writes slot {d}")
            elif prev is not None:
                for d in range(D):
                    if d != hd:
                        hp.same(g["ring"][b, d], prev["ring"][b, d], f"call {k} env {b}: a push leaves slot {d}")
            u = sr.pixel_uniforms(dc.BIG_OFFSET + b, frame, dc.SEED, h * w)
            far, edge, drop = sr.masks(z[b], p, u[:, 2])
            lost = edge | drop
            hp.same(v[far], np.full(int(far.sum()), F32(FAR)), f"call {k} env {b}: far pixels")
            hp.same(v[lost], np.full(int(lost.sum()), F32(-1.0)), f"call {k} env {b}: lost pixels")
            keep = ~far & ~lost
            assert not np.any(v[keep] == F32(-1.0)), (k, b)
            zn, n, rad, sigma = sr.noisy(z[b], p, u)
            bar = sr.value_bar(z[b], n, rad, sigma)
            err = np.abs(v.astype(np.float64) - v64[b])
            ratio = float((err[keep] / bar[keep]).max())
            worst, kept = max(worst, ratio), kept + int(keep.sum())
            assert np.all(err[keep] <= bar[keep]), (k, b, ratio)
            assert np.all((v[keep] >= p.near) & (v[keep] <= p.far))
        prev = g
    print(f"{h}x{w}: worst |v - v_ref| / bar over {kept} kept pixels: {worst:.3f}")
    assert kept > 15 * h * w  # 31 env images were sensed: about half of their pixels, at the least, were judged
    lat = ref[0][1]["latency"]
    assert lat.tolist() == [0, 1, 0, 2, 0]  # every delay of [0, 2] was run


@pytest.mark.parametrize("h,w", SIZES)
def test_noise_and_quantisation_differ_by_one_step_near_half_steps_only(sim, h, w):
    p = sr.params(w, h, far=FAR, latency=(0, 2), invalid_value=-1.0, quant=0.01, edge_thresh=0.1, dropout_p=0.02,
                  **NOISE)
    z = _exact(1, h, w)
    st = _alloc(N, p)
    _flags(sim, ())
    assert _sense(sim, p, sr.FILL, 6, hp.dev(z), st) == 0
    g = _np(st)
    q = float(p.quant)
    off = total = 0
    for b in range(N):
        u = sr.pixel_uniforms(dc.BIG_OFFSET + b, 6, dc.SEED, h * w)
        far, edge, drop = sr.masks(z[b], p, u[:, 2])
        keep = ~far & ~(edge | drop)
        zn, n, rad, sigma = sr.noisy(z[b], p, u)
        bar = sr.value_bar(z[b], n, rad, sigma) + 2.0 ** -22  # (+ the roundings of the division and the product)
        t = zn / np.float64(p.quant)
        near_half = np.abs(t - np.floor(t) - 0.5) * np.float64(p.quant) <= bar
        v, vref = g["sensed"][b].astype(np.float64), sr.sense(z[b], p, u)
        hp.same(g["sensed"][b][~keep], vref[~keep].astype(F32), f"env {b}: far and lost pixels")
        same = np.abs(v - vref) <= 2.0 ** -22 * FAR
        one_off = np.abs(np.abs(v - vref) - q) <= 2.0 ** -21 * FAR
        assert np.all(same[keep] | (one_off[keep] & near_half[keep])), (b, np.argwhere(keep & ~same)[:5])
        off, total = off + int((keep & ~same).sum()), total + int(keep.sum())
        assert (keep & near_half).sum() < 0.01 * h * w
    print(f"{h}x{w}: {off} of {total} kept pixels one step off the reference")


def test_injected_uniforms_clamp_and_dropout_threshold(sim):
    h, w = SIZES[0]
    prob = F32(0.25)
    p = sr.params(w, h, far=FAR, latency=(0, 0), invalid_value=-1.0, dropout_p=prob, **NOISE)
    z = _exact(0, h, w)
    rng = np.random.default_rng(5)
    u = rng.random((N, h, w, 3)).astype(F32)
    u[..., 2] = F32(0.5)
    u[:, :, 0::4, 0] = F32(0.0)                              # u0 = 0: the clamp at 1e-7
    u[:, :, 1::4, 2] = np.nextafter(prob, F32(0.0))          # just below dropout_p: lost
    u[:, :, 2::4, 2] = prob                                  # at it: kept (the test is a strict <)
    u[:, :, 3::4, 2] = np.nextafter(prob, F32(1.0))          # just above: kept
    st = _alloc(N, p)
    _flags(sim, ())
    assert _sense(sim, p, sr.FILL, 3, hp.dev(z), st, uniforms=hp.dev(u)) == 0
    g = _np(st)
    np.testing.assert_array_equal(g["latency"], 0)
    clamped = 0
    for b in range(N):
        far, edge, drop = sr.masks(z[b], p, u[b, ..., 2])
        assert not edge.any() and np.array_equal(drop[:, 1::4], ~far[:, 1::4]) and not drop[:, 0::4].any()
        assert not drop[:, 2::4].any() and not drop[:, 3::4].any()
        v = g["sensed"][b]
        hp.same(v[drop], np.full(int(drop.sum()), F32(-1.0)), "dropped")
        hp.same(v[far], np.full(int(far.sum()), F32(FAR)), "far")
        keep = ~far & ~drop
        zn, n, rad, sigma = sr.noisy(z[b], p, u[b])
        err = np.abs(v.astype(np.float64) - sr.sense(z[b], p, u[b]))
        assert np.all(err[keep] <= sr.value_bar(z[b], n, rad, sigma)[keep]), b
        first = keep[:, 0::4]
        assert np.allclose(rad[:, 0::4][first], np.sqrt(-2.0 * np.log(np.float64(F32(1e-7)))))
        clamped += int(first.sum())
        assert np.isfinite(v).all()
    assert clamped > 100


def test_sub_range_and_determinism(sim):
    h, w = SIZES[1]
    p = sr.params(w, h, far=FAR, latency=(0, 2), invalid_value=-1.0, edge_thresh=0.1, dropout_p=0.02, quant=0.001,
                  **NOISE)
    z = hp.dev(_exact(2, h, w))
    _flags(sim, (2,))
    full = _alloc(N, p)
    assert _sense(sim, p, sr.FILL, 5, z, full) == 0
    assert _sense(sim, p, sr.PUSH, 6, z, full) == 0
    # two identical calls from a copied state: bit-identical
    a = {k: full[k].clone() for k in KEYS}
    b = {k: full[k].clone() for k in KEYS}
    assert _sense(sim, p, sr.PUSH, 7, z, a) == 0 and _sense(sim, p, sr.PUSH, 7, z, b) == 0
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
    assert not torch.equal(a["sensed"], full["sensed"]) or not torch.equal(a["ring"], full["ring"])
    # envs [1, 4) into rows 1..3 of poisoned arrays: rows 0 and 4 stay, rows 1..3 are the full call's
    part = _alloc(N, p)
    assert _sense(sim, p, sr.FILL, 5, z, part, first=1, count=3, row=1) == 0
    assert _sense(sim, p, sr.PUSH, 6, z, part, first=1, count=3, row=1) == 0
    for key in KEYS:
        assert bool((part[key][0] == -7).all()) and bool((part[key][4] == -7).all()), key
        assert torch.equal(part[key][1:4], full[key][1:4]), key
    assert int(full["head"][2]) == 0 and int(full["head"][1]) == 1  # (env 2 was flagged: the push refilled it)
    # a count of zero is accepted and writes nothing
    assert _sense(sim, p, sr.PUSH, 8, z, part, first=5, count=0, row=0) == 0
    assert bool((part["sensed"][0] == -7).all())


def test_refusals_leave_the_arrays_alone(sim):
    h, w = 12, 16
    L = sim.L
    z = hp.dev(_exact(0, h, w))
    st = _alloc(N, sr.params(w, h, latency=(0, 15)))  # (room for every latency_max a refused call names)

    def call(sim_=True, sensor=True, null=None, first=0, count=N, mode=sr.FILL, **kw):
        s = _struct(sr.params(w, h, far=FAR, latency=(0, 1)))
        for key, v in kw.items():
            setattr(s, key, v)
        ptr = {k: None if k == null else hp.vp(t) for k, t in dict(st, depth=z).items()}
        return L.lrl_sim_depth_sense(sim.h if sim_ else None, C.byref(s) if sensor else None, first, count, mode,
                                     C.c_uint64(1), ptr["depth"], None, ptr["ring"], ptr["head"], ptr["latency"],
                                     ptr["sensed"], hp.stream())
    inf, nan = float("inf"), float("nan")
    bad = [dict(sim_=False), dict(sensor=False)] + [dict(null=k) for k in ("depth",) + KEYS] + \
          [dict(first=-1), dict(first=1, count=N), dict(first=N + 1, count=0), dict(count=-1), dict(count=N + 1),
           dict(width=0), dict(width=1025), dict(height=0), dict(height=1025),
           dict(near=-0.01), dict(near=FAR), dict(near=4.0), dict(far=3.0e38), dict(far=inf), dict(far=nan),
           dict(near=nan)] + \
          [{k: v} for k in ("noise_a", "noise_b", "edge_thresh", "quant") for v in (-1e-6, inf, nan)] + \
          [dict(dropout_p=-0.01), dict(dropout_p=1.01), dict(dropout_p=nan), dict(invalid_value=inf),
           dict(invalid_value=-inf), dict(invalid_value=nan), dict(latency_min=-1), dict(latency_min=2, latency_max=1),
           dict(latency_max=16), dict(mode=-1), dict(mode=3)]
    _flags(sim, (0, 1, 2, 3, 4))
    for kw in bad:
        L.lrl_set_error(0, b"")
        assert call(**kw) == -1, kw
        assert len(L.lrl_last_error()) > 0, kw
    hp.sync()
    for key in KEYS:
        assert bool((st[key] == -7).all()), key
    assert call(dropout_p=1.0, noise_a=0.0, quant=0.0, edge_thresh=0.0, latency_max=15) == 0  # the ends are inside
    hp.sync()
    assert bool((st["sensed"] != -7).all()) and bool((st["head"] == 0).all())
    _flags(sim, ())


# ---- LeggedRobotEnv with the group -----------------------------------------------------------------------------------
CHASE = dict(pos=(-0.55, 0.05, 0.35), pitch_deg=30.0)  # behind and above the trunk: the robot fills the image


def _env(n, interval, device_resets, seed=7, sensor=True, camera=True, w=16, h=12, **sensor_kw):
    from lrl.env import LeggedRobotEnv
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = n
    if camera:
        lcfg.add_depth_camera(cfg, width=w, height=h, update_interval=interval, **CHASE)
    if sensor:
        lcfg.add_depth_sensor(cfg, **sensor_kw)
    env = LeggedRobotEnv(DEV, cfg=cfg, seed=seed, legacy_fork=False, device_resets=device_resets)
    env.reset()
    return env


ZERO = dict(noise_a=0.0, noise_b=0.0, dropout_p=0.0, edge_thresh=0.0, quant=0.0)


@pytest.mark.parametrize("device_resets", [True, False])
def test_step_hookup_delivers_the_previous_refresh(device_resets):
    a = _env(5, 3, device_resets, latency_frames=[1, 1], **ZERO)
    b = _env(5, 3, device_resets, sensor=False)
    try:
        assert a._dev_path == device_resets and not hasattr(b, "depth_sensed") and b._depth_sensor is None
        assert a.depth_sensed.shape == (5, 12, 16) and a.depth_sensed.dtype == torch.float32
        assert a.depth_latency.dtype == torch.int32 and a._depth_ring.shape == (5, 2, 12, 16)
        # reset() took the first tick: a fill of every env, so the sensed image is the exact one
        assert a._depth_step == 1 and torch.equal(a.depth_sensed, a.depth_images)
        assert bool((a.depth_latency == 1).all())
        expect = a.depth_images.clone()  # per env: the frame a full refresh must deliver next
        gen = torch.Generator(device=DEV).manual_seed(11)
        refills = 0
        for k in range(1, 11):
            if k in (4, 6):  # an off-interval step and a full refresh: an env runs into its time-out in it
                for e in (a, b):
                    e.episode_length_buf[2 if k == 4 else 3] = int(e.max_episode_length)
            act = torch.rand(5, 12, device=DEV, generator=gen) * 2 - 1
            before = a.depth_sensed.clone()
            oa, ra, da, xa = a.step(act)
            ob, rb, db, xb = b.step(act)
            for x, y in ((oa, ob), (xa["privileged_obs"], xb["privileged_obs"]), (ra, rb), (da, db),
                         (a.root_states, b.root_states), (a.depth_images, b.depth_images)):
                assert torch.equal(x, y), k
            assert a.depth_refreshed == b.depth_refreshed == (k % 3 == 0)
            flag = da.bool()
            if k in (4, 6):
                assert bool(flag[2 if k == 4 else 3])
            if a.depth_refreshed:
                # the previous full refresh's image; for an env reset since then its redraw (at this step: this image)
                assert torch.equal(a.depth_sensed[~flag], expect[~flag]), k
                assert torch.equal(a.depth_sensed[flag], a.depth_images[flag]), k
                assert bool((a.depth_sensed[~flag] != a.depth_images[~flag]).any()), k  # ... really a frame late
                expect = a.depth_images.clone()
            else:
                assert torch.equal(a.depth_sensed[~flag], before[~flag]), k
                assert torch.equal(a.depth_sensed[flag], a.depth_images[flag]), k
                expect[flag] = a.depth_images[flag]
            refills += int(flag.sum())
        assert refills >= 2
        # render_depth keeps its meaning: the exact image now, the sensor untouched
        sensed, step = a.depth_sensed.clone(), a._depth_step
        d, _ = a.render_depth()
        assert d is a.depth_images and torch.equal(a.depth_sensed, sensed) and a._depth_step == step
    finally:
        a.close()
        b.close()


def test_step_hookup_with_the_default_model_is_deterministic_and_noisy():
    a, b = _env(5, 2, None, seed=9), _env(5, 2, None, seed=9)
    try:
        gen = torch.Generator(device=DEV).manual_seed(13)
        for _ in range(4):
            act = torch.rand(5, 12, device=DEV, generator=gen) * 2 - 1
            a.step(act)
            b.step(act)
            assert torch.equal(a.depth_sensed, b.depth_sensed) and torch.equal(a.depth_latency, b.depth_latency)
        assert not torch.equal(a.depth_sensed, a.depth_images)
        far = float(a.cfg.depth.far)
        assert bool(((a.depth_sensed >= float(a.cfg.depth.near)) & (a.depth_sensed <= far)).all())
        assert bool(((a.depth_latency >= 0) & (a.depth_latency <= 1)).all())
    finally:
        a.close()
        b.close()


def test_python_side_refusals():
    with pytest.raises(ValueError, match=r"depth_sensor.*Cfg\.depth|Cfg\.depth.*depth_sensor"):
        _env(5, 3, None, camera=False)
    with pytest.raises(ValueError, match="latency_frames"):
        _env(5, 3, None, latency_frames=[2, 1])
    with pytest.raises(ValueError, match="latency_frames"):
        _env(5, 3, None, latency_frames=[0, 16])
    with pytest.raises(RuntimeError, match="dropout_p"):  # the library's own refusal surfaces at the first tick
        _env(5, 3, None, dropout_p=1.5)


def test_distiller_reads_the_sensed_images():
    from lrl import vision
    from lrl.env import LeggedRobotEnv

    def make(sensor):
        cfg = ds.go1_trimesh_cfg(4)  # (tests/test_vision_gpu.py's env: the rough trimesh with the height scan)
        cfg.terrain.measure_heights = True
        cfg.env.num_observations = 42 + len(cfg.terrain.measured_points_x) * len(cfg.terrain.measured_points_y)
        lcfg.add_depth_camera(cfg, width=16, height=16, update_interval=1, **CHASE)
        if sensor:
            lcfg.add_depth_sensor(cfg, invalid_value=0.0, dropout_p=0.2)
        env = LeggedRobotEnv(DEV, cfg=cfg, seed=ds.TERRAIN_SEED)
        env.reset()
        return env
    env = make(True)
    try:
        first, scan = vision.scan_columns(env)
        enc = vision.DepthEncoder(16, 16, scan, extra_dim=first, hidden=16).to(DEV)
        obs = env.step(torch.zeros(4, 12, device=DEV))[0]
        d = vision.DepthDistiller(env, enc, capacity=8, batch_size=4, sensed=True)
        d.collect(obs)
        assert torch.equal(d.images[:4], env.depth_sensed) and not torch.equal(d.images[:4], env.depth_images)
        exact = vision.DepthDistiller(env, enc, capacity=8, batch_size=4)
        exact.collect(obs)
        assert torch.equal(exact.images[:4], env.depth_images)
        img = env.depth_sensed
        want = enc.forward_native(img, obs[:, :first]) if d.native else enc(img, obs[:, :first])
        assert torch.equal(d.predict_obs(obs)[:, first:], want.detach())
    finally:
        env.close()
    env = make(False)
    try:
        with pytest.raises(ValueError, match="add_depth_sensor"):
            vision.DepthDistiller(env, enc, capacity=8, batch_size=4, sensed=True)
    finally:
        env.close()
