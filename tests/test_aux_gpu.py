"""The non-step env kernels (csrc/lrl_aux.hip and observe_kernel of csrc/lrl_env_dispatch.hip) against the independent
references of tests/aux_ref.py, through the C ABI on sims made with lrl_sim_create.

Forward kinematics (rigid_body_kernel, the foot rows of extras_snapshot_kernel) is held to ``aux_ref.fk`` in float64.
The bar is not taken from the kernel: ``fk`` is evaluated in float32 numpy on the test's own inputs (both robots and
Go1 with random fixed joint rotations and axes, 67 + 1 envs each), its worst deviation from float64 is taken per
quantity and per position scale, and the bar is 4 x that deviation (a different operation order and the device
sincosf).  Measured (the deviation on the CPU, the kernel on an MI355X; bar = 4 x the float32 deviation; the kernel's
worst error over every case of the input sets within 1 m and within 100 m of the origin):

    quantity                   inputs    float32 deviation   bar         kernel's worst error
    position (m)               1 m       2.179e-07           8.717e-07   1.829e-07
    position (m)               100 m     1.230e-05           4.921e-05   1.230e-05
    rotation entries           1 m       6.478e-07           2.591e-06   4.135e-07
    rotation entries           100 m     6.818e-07           2.727e-06   4.018e-07
    linear velocity (m/s)      1 m       5.797e-06           2.319e-05   3.338e-06
    linear velocity (m/s)      100 m     6.078e-06           2.431e-05   2.935e-06
    angular velocity (rad/s)   1 m       1.768e-05           7.074e-05   9.885e-06
    angular velocity (rad/s)   100 m     9.972e-06           3.989e-05   7.739e-06
    extras' foot rows (m)      1 m       (position's)        8.717e-07   1.829e-07
    extras' foot rows (m)      100 m     (position's)        4.921e-05   1.230e-05

Everything else is exact: id lists, step codes, history shifts, setters and the counter-RNG draws are compared bit for
bit (the RNG against the Philox restatement that test_aux_ref.py pins on the Random123 known answers), the episode
means within the rounding bound of their reduction.  No test passes an env id outside [0, n).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import aux_ref as ar
from helpers import DEV, dev, make, make_rough, mc_sim, npy, robot_table, same, sim_of, stream, sync, vp
from lrl import _abi

pytestmark = pytest.mark.gpu

F32 = np.float32
i32, i64, f32c, u32c = C.c_int32, C.c_int64, C.c_float, C.c_uint32


@functools.lru_cache(None)
def _rough():
    return make_rough()


def rough_sim(n, offset=0, seed=1):
    _, _, M, P = _rough()
    return sim_of(M, P, n, offset, seed)


def set_gentle_terrain(s, G=120):
    """A G x G vertex grid of centimetre-high bumps for a rough sim (lrl_sim_step needs a mesh); world x, y from
    -border_size to (G - 1) horizontal_scale - border_size."""
    hs, vs = s.P.horizontal_scale, s.P.vertical_scale
    i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    samples = np.round(0.05 * np.sin(0.7 * i * hs) * np.cos(0.5 * j * hs) / vs).astype(np.int16)
    vtx = np.stack([i * hs, j * hs, samples.astype(np.float64) * vs], -1).reshape(-1, 3).astype(F32)
    samples = np.ascontiguousarray(samples)
    _abi.check(s.L.lrl_sim_set_terrain(s.h, vtx.ctypes.data_as(C.c_void_p), samples.ctypes.data_as(C.c_void_p),
                                       i32(G), i32(G)))


# =================================================================================================================
# Forward kinematics
# =================================================================================================================
MODELS = ("mc", "go1", "go1_random_joints")
FK_QUANTITIES = ("pos", "rot", "vel", "ang")


def _table(name):
    """(reference table in float64 of the float32 values the device gets, lrl_model, params)."""
    return robot_table(name)


@functools.lru_cache(None)
def _fk_inputs(name, n, scale):
    rng = np.random.default_rng([MODELS.index(name), n, int(scale)])
    M = _table(name)[1]
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    if n >= 6:  # exact and near half turns about x, y, z
        s, c = np.sin((np.pi - 1e-3) / 2), np.cos((np.pi - 1e-3) / 2)
        quat[:6] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [s, 0, 0, c], [0, s, 0, c], [0, 0, s, c]]
    root = np.zeros((n, 13))
    root[:, 0:3] = rng.uniform(-scale, scale, (n, 3))
    root[:, 3:7] = quat
    root[:, 7:10] = rng.uniform(-3, 3, (n, 3))
    root[:, 10:13] = rng.uniform(-6, 6, (n, 3))
    lo = np.minimum(np.array(M.dof_lower[:]), -1.0) - 0.3
    hi = np.maximum(np.array(M.dof_upper[:]), 1.0) + 0.3
    q, qd = rng.uniform(lo, hi, (n, 12)), rng.uniform(-20, 20, (n, 12))
    com = rng.uniform(-0.1, 0.1, (n, 3))
    return tuple(a.astype(F32) for a in (root, com, q, qd))


@functools.lru_cache(None)
def _fk_ref(name, n, scale):
    """fk in float64 for every env of the inputs, and the worst |float32 fk - float64 fk| per quantity."""
    model = _table(name)[0]
    root, com, q, qd = _fk_inputs(name, n, scale)
    ev = lambda dt: [np.stack(x) for x in zip(*(ar.fk(model, root[e], com[e], q[e], qd[e], dt) for e in range(n)))]
    r64, r32 = ev(np.float64), ev(np.float32)
    assert all(x.dtype == np.float32 for x in r32)
    return dict(zip(FK_QUANTITIES, r64)), {k: float(np.abs(a.astype(np.float64) - b).max())
                                            for k, a, b in zip(FK_QUANTITIES, r32, r64)}


@functools.lru_cache(None)
def fk_deviation(scale):
    """Worst float32 deviation of fk per quantity over every input set of this position scale."""
    devs = [_fk_ref(name, n, scale)[1] for name in MODELS for n in (67, 1)]
    return {k: max(d[k] for d in devs) for k in FK_QUANTITIES}


def _quat_mats(q):
    return np.stack([ar.quat_to_mat(x) for x in q.reshape(-1, 4).astype(np.float64)]).reshape(q.shape[:-1] + (3, 3))


def test_fk_inputs_take_every_quaternion_branch():
    """CPU side of the coverage condition: over the (env, body) pairs of each 67-env input set the reference rotation
    falls, at least 1e-4 clear of the boundaries, into each of the four branches of the matrix-to-quaternion
    conversion."""
    for name in MODELS:
        for scale in (1.0, 100.0):
            rot = _fk_ref(name, 67, scale)[0]["rot"]
            taken = {b for b, margin in (ar.quat_mat_branch(R) for R in rot.reshape(-1, 3, 3)) if margin > 1e-4}
            assert taken == {0, 1, 2, 3}, (name, scale, taken)


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("n", [67, 1])
@pytest.mark.parametrize("name", MODELS)
def test_rigid_body_state_and_extras_match_fk(name, n, scale):
    model, M, P = _table(name)
    root, com, q, qd = _fk_inputs(name, n, scale)
    ref = _fk_ref(name, n, scale)[0]
    deviation = fk_deviation(scale)
    bar = {k: 4.0 * v for k, v in deviation.items()}
    rng = np.random.default_rng(5)
    B = M.num_bodies
    feet = list(P.feet[: P.num_feet])
    with sim_of(M, P, n) as s:
        s.t(_abi.T_ROOT_STATE).copy_(dev(root))
        s.t(_abi.T_COM_DISPLACEMENT).copy_(dev(com))
        s.t(_abi.T_DOF_POS).copy_(dev(q))
        s.t(_abi.T_DOF_VEL).copy_(dev(qd))
        live = {}
        for tid, cols in ((_abi.T_JOINT_POS_TARGET, 12), (_abi.T_TORQUES, 12), (_abi.T_BASE_LIN_VEL, 3),
                          (_abi.T_BASE_ANG_VEL, 3), (_abi.T_COMMANDS, 4)):
            live[tid] = rng.uniform(-9, 9, (n, cols)).astype(F32)
            s.t(tid).copy_(dev(live[tid]))
        contact = rng.uniform(-5, 5, (n, B, 3)).astype(F32)
        edge = np.array([1.0, np.nextafter(F32(1), F32(2)), 0.0, 5.0, -3.0, np.nextafter(F32(1), F32(0))], F32)
        for e in range(n):
            for f, b in enumerate(feet):
                contact[e, b, 2] = edge[(e + f) % 6]
        s.t(_abi.T_CONTACT_FORCE).copy_(dev(contact))
        _abi.check(s.L.lrl_sim_refresh_rigid_body_state(s.h, stream()))
        snap = torch.full((77, n), -77.0, device=DEV)
        _abi.check(s.L.lrl_sim_extras_snapshot(s.h, vp(snap), stream()))
        sync()
        rb = npy(s.t(_abi.T_RIGID_BODY_STATE)).astype(np.float64)
        snap = npy(snap)
    assert rb.shape == (n, B, 13)
    err = {"pos": np.abs(rb[..., 0:3] - ref["pos"]).max(), "vel": np.abs(rb[..., 7:10] - ref["vel"]).max(),
           "ang": np.abs(rb[..., 10:13] - ref["ang"]).max(),
           "rot": np.abs(_quat_mats(rb[..., 3:7]) - ref["rot"]).max()}
    foot_err = np.abs(snap[50:62].astype(np.float64).reshape(4, 3, n).transpose(2, 0, 1)[:, : len(feet)]
                      - ref["pos"][:, feet]).max()
    for k in FK_QUANTITIES:
        print(f"fk {name} n={n} scale={scale:g} {k}: float32 deviation {deviation[k]:.3e} bar {bar[k]:.3e} "
              f"kernel {err[k]:.3e}")
    print(f"fk {name} n={n} scale={scale:g} extras foot rows: kernel {foot_err:.3e}")
    for k in FK_QUANTITIES:
        assert err[k] <= bar[k], (k, err[k], bar[k])
    assert foot_err <= bar["pos"], (foot_err, bar["pos"])
    # a unit quaternion: |q|^2 moves by at most about 6 x the error of the matrix entries (a dominant component of at
    # least 1/2 keeps every partial derivative below 1), so |q| by 3 x, plus its own few roundings
    assert np.abs(np.linalg.norm(rb[..., 3:7], axis=-1) - 1).max() <= 4 * bar["rot"]
    # every other row of the snapshot is a copy
    same(snap[0:12], q.T, "dof_pos rows")
    same(snap[12:24], qd.T, "dof_vel rows")
    same(snap[24:36], live[_abi.T_JOINT_POS_TARGET].T, "joint_pos_target rows")
    same(snap[36:39], live[_abi.T_BASE_LIN_VEL].T, "base_lin_vel rows")
    same(snap[39:42], live[_abi.T_BASE_ANG_VEL].T, "base_ang_vel rows")
    same(snap[42:46], live[_abi.T_COMMANDS].T, "command rows")
    same(snap[62:65], root[:, 0:3].T, "base position rows")
    same(snap[65:77], live[_abi.T_TORQUES].T, "torque rows")
    want = np.zeros((4, n), F32)
    for f, b in enumerate(feet):
        want[f] = contact[:, b, 2] > F32(1.0)
    same(snap[46:50], want, "contact rows (force z > 1, strictly)")
    assert want.min() == 0 and want.max() == 1


# =================================================================================================================
# compact_kernel and step_code_kernel
# =================================================================================================================
def _flag_patterns(n, rng):
    per = (n + 1023) // 1024
    run = np.zeros(n, np.uint8)
    a = n // 3
    run[a: a + 3 * per + 2] = 1  # longer than a thread's share, across thread boundaries
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 1
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "first": first, "last": last, "run": run,
            "random 3 %": (rng.random(n) < 0.03).astype(np.uint8), "random 50 %": (rng.random(n) < 0.5).astype(np.uint8)}


def _env_lists(s, mode, interval, ids_out, count_out):
    return s.L.lrl_sim_env_lists(s.h, i32(mode), i32(interval), vp(ids_out), vp(count_out), stream())


def _check_list(ids_out, count_out, want, what):
    sync()
    ids, count = npy(ids_out), int(npy(count_out)[0])
    assert count == len(want), (what, count, len(want))
    same(ids[:count], want, what)
    assert (ids[count:] == -7).all(), f"{what}: wrote past the count"


@pytest.mark.parametrize("n", [1, 67, 1023, 1024, 1025, 2049, 4097])
def test_env_lists_match_flatnonzero(n):
    rng = np.random.default_rng(n)
    with mc_sim(n) as s:
        reset, eplen = s.t(_abi.T_RESET), s.t(_abi.T_EPISODE_LENGTH)
        pad = 9
        fresh = lambda: (torch.full((n + pad,), -7, dtype=torch.int32, device=DEV),
                         torch.full((1,), -9, dtype=torch.int32, device=DEV))
        host = torch.full((3 * n + pad,), -5.0).pin_memory()
        lens = rng.integers(0, 50, n).astype(np.int32)
        eplen.copy_(dev(lens, torch.int32))
        for what, flags in _flag_patterns(n, rng).items():
            reset.copy_(dev(flags, torch.uint8))
            ids_out, count_out = fresh()
            _abi.check(_env_lists(s, 0, 5, ids_out, count_out))
            _check_list(ids_out, count_out, ar.env_list(0, flags, lens, 5), f"mode 0, {what}")
            # the reset list of lrl_sim_step_code is the same compaction, without a count
            ids_out, _ = fresh()
            host.fill_(-5.0)
            _abi.check(s.L.lrl_sim_step_code(s.h, i32(5), i32(-1), i32(-1), vp(host), vp(ids_out), stream()))
            sync()
            want = ar.env_list(0, flags, lens, 5)
            same(npy(ids_out)[: len(want)], want, f"step_code list, {what}")
            assert (npy(ids_out)[len(want):] == -7).all()
            same(host.numpy()[:n], ar.step_code(flags, lens, 5), f"step code, {what}")
            assert (host.numpy()[n:] == -5.0).all()
        reset.zero_()
        for interval in (1, 3, 7):
            ids_out, count_out = fresh()
            _abi.check(_env_lists(s, 1, interval, ids_out, count_out))
            want = ar.env_list(1, None, lens, interval)
            assert len(want) == n if interval == 1 else 0 < len(want) < n or n < 8
            _check_list(ids_out, count_out, want, f"mode 1, interval {interval}")
        big = lens.copy()
        big[rng.random(n) < 0.4] = 2 ** 31 - 2
        big[-1] = 2 ** 31 - 2
        eplen.copy_(dev(big, torch.int32))
        ids_out, count_out = fresh()
        _abi.check(_env_lists(s, 1, 2 ** 31 - 1, ids_out, count_out))
        _check_list(ids_out, count_out, np.flatnonzero(big == 2 ** 31 - 2).astype(np.int32), "mode 1, interval 2^31 - 1")


def test_env_lists_refuses_bad_arguments():
    with mc_sim(67) as s:
        s.t(_abi.T_RESET).fill_(1)
        ids_out = torch.full((67,), -7, dtype=torch.int32, device=DEV)
        count_out = torch.full((1,), -9, dtype=torch.int32, device=DEV)
        assert _env_lists(s, 0, 0, ids_out, count_out) != 0
        assert _env_lists(s, 1, 0, ids_out, count_out) != 0
        assert _env_lists(s, 1, -3, ids_out, count_out) != 0
        assert _env_lists(s, 2, 5, ids_out, count_out) != 0
        assert _env_lists(s, -1, 5, ids_out, count_out) != 0
        assert _env_lists(s, 0, 5, None, count_out) != 0
        assert _env_lists(s, 0, 5, ids_out, None) != 0
        sync()
        assert (npy(ids_out) == -7).all() and npy(count_out)[0] == -9


@pytest.mark.parametrize("n", [67, 1025])
def test_step_code(n):
    rng = np.random.default_rng(100 + n)
    with mc_sim(n) as s:
        sums = s.t(_abi.T_COMMAND_SUMS)
        ncs = sums.shape[0]
        table = rng.uniform(-50, 50, (ncs, n)).astype(F32)
        sums.copy_(dev(table))
        flags = (rng.random(n) < 0.3).astype(np.uint8)
        lens = rng.integers(0, 40, n).astype(np.int32)
        s.t(_abi.T_RESET).copy_(dev(flags, torch.uint8))
        s.t(_abi.T_EPISODE_LENGTH).copy_(dev(lens, torch.int32))
        host = torch.empty(3 * n + 11).pin_memory()
        call = lambda interval, r0, r1: s.L.lrl_sim_step_code(s.h, i32(interval), i32(r0), i32(r1), vp(host), None,
                                                              stream())
        for interval in (1, 3, 7):
            for r0, r1 in ((2, ncs - 1), (ncs - 1, 0)):
                host.fill_(-5.0)
                _abi.check(call(interval, r0, r1))
                got = host.numpy()
                code = ar.step_code(flags, lens, interval)
                assert set(np.unique(code)) <= {0.0, 1.0, 2.0, 3.0} and (interval != 1 or (code >= 2).all())
                same(got[:n], code, "code")
                same(got[n: 2 * n], table[r0], "first sum row")
                same(got[2 * n: 3 * n], table[r1], "second sum row")
                assert (got[3 * n:] == -5.0).all()
            host.fill_(-5.0)
            _abi.check(call(interval, -1, -1))
            same(host.numpy()[:n], ar.step_code(flags, lens, interval), "code alone")
            assert (host.numpy()[n:] == -5.0).all()
        host.fill_(-5.0)
        for interval, r0, r1 in ((3, -1, 2), (3, 2, -1), (3, ncs, 0), (3, 0, ncs), (0, 0, 1), (0, -1, -1)):
            assert call(interval, r0, r1) != 0, (interval, r0, r1)
        sync()
        assert (host.numpy() == -5.0).all()
        same(npy(sums), table, "command sums untouched")


# =================================================================================================================
# rows_mean_zero_kernel
# =================================================================================================================
COLS = 4096
ID_COUNTS = (1, 2, 255, 256, 257, 1000, 4096)


def _mixed(rng, shape):
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F32)


def _mean_bound(n, absmean):
    # at most ceil(n / 256) - 1 serial additions, 8 tree levels and one division on the way of every element
    return (np.ceil(n / 256) + 10) * 2.0 ** -24 * absmean


def _table_with_padding(rng, rows, ld):
    tab = np.full((rows, ld), -12345.0, F32)
    tab[:, :COLS] = _mixed(rng, (rows, COLS))
    return tab


def _check_means(tab0, tab1, means, ids, zero, what):
    """means against the float64 means of tab0 over ids; tab1 (the table afterwards) zeroed exactly there."""
    want, absmean = ar.row_means(tab0, ids)
    err = np.abs(means.astype(np.float64) - want)
    assert (err <= _mean_bound(len(ids), absmean)).all(), (what, err.max(), _mean_bound(len(ids), absmean).min())
    after = tab0.copy()
    if zero:
        after[:, ids] = 0.0
    same(tab1, after, f"{what}: table")


@pytest.mark.parametrize("pad", [0, 61])
@pytest.mark.parametrize("rows", [1, 23])
def test_rows_mean_zero_host_count(rows, pad):
    L = _abi.lib()
    rng = np.random.default_rng(rows * 100 + pad)
    ld = COLS + pad
    for k in ID_COUNTS:
        for zero in (0, 1):
            tab0 = _table_with_padding(rng, rows, ld)
            ids = rng.permutation(COLS)[:k].astype(np.int32)
            tab, dids = dev(tab0), dev(ids, torch.int32)
            means = torch.full((rows + 3,), -3.0, device=DEV)
            assert L.lrl_rows_mean_zero(vp(tab), i64(ld), i32(rows), vp(dids), i32(k), vp(means), i32(zero),
                                        stream()) == 0
            sync()
            m = npy(means)
            assert (m[rows:] == -3.0).all()
            _check_means(tab0, npy(tab), m[:rows], ids, zero, f"rows {rows} ld {ld} ids {k} zero {zero}")


def test_rows_mean_zero_host_edges():
    L = _abi.lib()
    rng = np.random.default_rng(3)
    tab0 = _table_with_padding(rng, 5, COLS)
    tab = dev(tab0)
    means = torch.full((5,), -3.0, device=DEV)
    ids = dev(np.arange(4), torch.int32)
    assert L.lrl_rows_mean_zero(vp(tab), i64(COLS), i32(5), None, i32(0), vp(means), i32(1), stream()) == 0
    sync()
    assert np.isnan(npy(means)).all()  # torch.mean of an empty selection
    means.fill_(-3.0)
    assert L.lrl_rows_mean_zero(vp(tab), i64(COLS), i32(0), vp(ids), i32(4), vp(means), i32(1), stream()) == 0
    assert L.lrl_rows_mean_zero(None, i64(COLS), i32(5), vp(ids), i32(4), vp(means), i32(1), stream()) != 0
    assert L.lrl_rows_mean_zero(vp(tab), i64(COLS), i32(5), vp(ids), i32(4), None, i32(1), stream()) != 0
    assert L.lrl_rows_mean_zero(vp(tab), i64(COLS), i32(5), None, i32(4), vp(means), i32(1), stream()) != 0
    assert L.lrl_rows_mean_zero(vp(tab), i64(COLS), i32(-1), vp(ids), i32(4), vp(means), i32(1), stream()) != 0
    sync()
    assert (npy(means) == -3.0).all()
    same(npy(tab), tab0, "table untouched")


@pytest.mark.parametrize("rows", [1, 23])
def test_rows_mean_zero_device_count(rows):
    L = _abi.lib()
    rng = np.random.default_rng(40 + rows)
    ld = COLS + 61
    prev0 = rng.uniform(-1, 1, rows).astype(F32)
    prev = dev(prev0)

    def run(nmax, count, with_prev, zero, ids_null=False):
        tab0 = _table_with_padding(rng, rows, ld)
        ids = rng.permutation(COLS)[:max(nmax, 1)].astype(np.int32)
        tab, dids, dcount = dev(tab0), dev(ids, torch.int32), dev([count], torch.int32)
        means = torch.full((rows + 3,), -3.0, device=DEV)
        assert L.lrl_rows_mean_zero_dev(vp(tab), i64(ld), i32(rows), None if ids_null else vp(dids), i32(nmax),
                                        vp(dcount), vp(means), vp(prev) if with_prev else None, i32(zero),
                                        stream()) == 0
        sync()
        m = npy(means)
        assert (m[rows:] == -3.0).all()
        return tab0, npy(tab), m[:rows], ids

    for nmax, count in ((1000, 300), (300, 257), (257, 1000), (256, 2 ** 31 - 1), (4096, 4096), (1, 1)):
        for zero in (0, 1):
            tab0, tab1, m, ids = run(nmax, count, True, zero)
            _check_means(tab0, tab1, m, ids[: min(nmax, count)], zero, f"nmax {nmax} count {count} zero {zero}")
    tab0, tab1, m, _ = run(500, 0, True, 1)  # an empty batch keeps the previous means
    same(m, prev0, "count 0 with prev")
    same(tab1, tab0, "count 0: table")
    tab0, tab1, m, _ = run(500, 0, False, 1)
    assert (m == -3.0).all()
    same(tab1, tab0, "count 0 without prev: table")
    tab0, tab1, m, _ = run(0, 7, True, 1, ids_null=True)  # the copy path
    same(m, prev0, "nmax 0 with prev")
    same(tab1, tab0, "nmax 0: table")
    tab0, tab1, m, _ = run(0, 7, False, 1, ids_null=True)
    assert (m == -3.0).all()


# =================================================================================================================
# shift_history_kernel
# =================================================================================================================
def _history_sim(kind, history, n):
    if kind == "rough":
        assert history == 15
        return rough_sim(n)
    try:
        _, _, M, P = make("mc", **{"env.num_observation_history": history})
    except Exception as e:  # the config layer may refuse a one- or two-row history
        pytest.skip(f"num_observation_history = {history} refused by the config layer: {e}")
    assert P.num_history == history
    return sim_of(M, P, n)


@pytest.mark.parametrize("n", [1, 67])
@pytest.mark.parametrize("kind,history", [("mc", 15), ("mc", 1), ("mc", 2), ("rough", 15)])
def test_shift_history(kind, history, n):
    with _history_sim(kind, history, n) as s:
        NO = s.P.num_obs
        assert NO == (229 if kind == "rough" else 42)
        H = NO * history
        hist, obs = s.t(_abi.T_OBS_HISTORY), s.t(_abi.T_OBS)
        assert tuple(hist.shape) == (n, H) and tuple(obs.shape) == (n, NO)
        old = (np.arange(n)[:, None] * H + np.arange(H)[None]).astype(F32)
        row = -(np.arange(n)[:, None] * NO + np.arange(NO)[None] + 1).astype(F32)
        assert old.max() < 2 ** 24 and -row.min() < 2 ** 24  # exact in float32
        hist.copy_(dev(old))
        obs.copy_(dev(row))
        _abi.check(s.L.lrl_sim_shift_history(s.h, stream()))
        sync()
        same(npy(hist), ar.shift_history(old, row), "lrl_sim_shift_history")
        same(npy(obs), row, "obs untouched")
        # HistoryWrapper.step: the shift launch before the env kernel, which writes the newest slot from its obs row
        if kind == "rough":
            set_gentle_terrain(s)
            s.t(_abi.T_ROOT_STATE)[:, 0:2] = 3.0
            s.t(_abi.T_ROOT_STATE)[:, 2] = 0.6
        hist.copy_(dev(old))
        actions = torch.zeros(n, 12, device=DEV)
        _abi.check(s.L.lrl_sim_step(s.h, vp(actions), u32c(_abi.STEP_HISTORY), stream()))
        sync()
        got, new = npy(hist), npy(obs)
        same(got[:, : H - NO], old[:, NO:], "step: shifted part")
        same(got[:, H - NO:], new, "step: newest slot")
        assert np.isfinite(new).all() and (new != row).any()


# =================================================================================================================
# observe_kernel
# =================================================================================================================
OBSERVED = (_abi.T_OBS, _abi.T_PRIV_OBS, _abi.T_OBS_HISTORY, _abi.T_BASE_LIN_VEL, _abi.T_BASE_ANG_VEL,
            _abi.T_PROJECTED_GRAVITY, _abi.T_LAST_ACTIONS, _abi.T_LAST_DOF_VEL, _abi.T_LAST_ROOT_VEL)


def _randomise_state(s, rng, xy):
    n, P = s.n, s.P
    root = np.zeros((n, 13), F32)
    root[:, 0:2] = rng.uniform(xy[0], xy[1], (n, 2))
    root[:, 2] = rng.uniform(0.3, 0.6, n)
    ang = rng.normal(size=(n, 3)) * 0.2
    th = np.linalg.norm(ang, axis=1, keepdims=True)
    root[:, 3:7] = np.concatenate([ang / th * np.sin(th / 2), np.cos(th / 2)], 1)
    root[:, 7:10] = rng.normal(size=(n, 3)) * 0.5
    root[:, 10:13] = rng.normal(size=(n, 3))
    s.t(_abi.T_ROOT_STATE).copy_(dev(root))
    s.t(_abi.T_DOF_POS).copy_(dev(np.array(P.default_dof_pos[:], F32)[None] + rng.normal(size=(n, 12)) * 0.2))
    s.t(_abi.T_DOF_VEL).copy_(dev(rng.normal(size=(n, 12))))
    s.t(_abi.T_COMMANDS).copy_(dev(rng.uniform(-1, 1, (n, 4))))
    s.t(_abi.T_PAYLOAD).copy_(dev(rng.uniform(-1, 3, n)))
    s.t(_abi.T_COM_DISPLACEMENT).copy_(dev(rng.uniform(-0.1, 0.1, (n, 3))))
    s.t(_abi.T_FRICTION).copy_(dev(rng.uniform(0.1, 4, n)))
    s.t(_abi.T_RESTITUTION).copy_(dev(rng.uniform(0, 1, n)))
    s.t(_abi.T_MOTOR_STRENGTH).copy_(dev(np.repeat(rng.uniform(0.9, 1.1, (n, 1)), 12, 1)))
    s.t(_abi.T_OBS_HISTORY).copy_(dev(rng.uniform(-1, 1, tuple(s.t(_abi.T_OBS_HISTORY).shape))))


@pytest.mark.parametrize("kind", ["mc plane", "go1 rough"])
def test_observe_rows_are_the_step_kernels(kind):
    n = 67
    rng = np.random.default_rng(17)
    with (mc_sim(n, seed=5) if kind == "mc plane" else rough_sim(n, seed=5)) as s:
        NO = s.P.num_obs
        assert s.P.add_noise and NO == (42 if kind == "mc plane" else 229)
        if kind == "go1 rough":
            set_gentle_terrain(s)
        _randomise_state(s, rng, (2.0, 6.0))
        flags = u32c(_abi.STEP_PHYSICS | _abi.STEP_HISTORY)
        actions = dev(rng.uniform(-1.5, 1.5, (n, 12)))
        _abi.check(s.L.lrl_sim_step(s.h, vp(actions), flags, stream()))
        sync()
        snap = {tid: npy(s.t(tid)).copy() for tid in OBSERVED}
        assert all(np.isfinite(v).all() for v in snap.values())
        assert len(np.unique(snap[_abi.T_OBS])) > n * NO // 2  # rows worth comparing
        H = snap[_abi.T_OBS_HISTORY].shape[1]
        same(snap[_abi.T_OBS_HISTORY][:, H - NO:], snap[_abi.T_OBS], "the step's newest history slot")
        written = (_abi.T_OBS, _abi.T_PRIV_OBS, _abi.T_BASE_LIN_VEL, _abi.T_LAST_ROOT_VEL)

        def sentinel():
            for tid in written:
                s.t(tid).fill_(-99.0)
            s.t(_abi.T_OBS_HISTORY)[:, H - NO:] = -99.0

        def check(ids, what):
            sync()
            rest = np.setdiff1d(np.arange(n), ids)
            for tid in OBSERVED:
                got = npy(s.t(tid))
                same(got[ids], snap[tid][ids], f"{what}: tensor {tid}, observed rows")
                if tid == _abi.T_OBS_HISTORY:
                    same(got[rest, : H - NO], snap[tid][rest, : H - NO], f"{what}: older history slots")
                    assert (got[rest, H - NO:] == -99.0).all(), f"{what}: newest slot of an env not listed"
                elif tid in written:
                    assert (got[rest] == -99.0).all(), f"{what}: tensor {tid}, rows of envs not listed"
                else:
                    same(got[rest], snap[tid][rest], f"{what}: tensor {tid}, rows of envs not listed")

        sentinel()
        every = dev(np.arange(n), torch.int32)
        _abi.check(s.L.lrl_sim_observe_idx(s.h, vp(every), i32(n), flags, stream()))
        check(np.arange(n), "every env")
        sentinel()
        some = rng.permutation(n)[:9].astype(np.int32)
        dsome = dev(some, torch.int32)
        _abi.check(s.L.lrl_sim_observe_idx(s.h, vp(dsome), i32(9), flags, stream()))
        check(some, "nine envs")
        for count, used in ((5, 5), (20, 9)):  # a device count below its bound, and one above it (clamped)
            sentinel()
            dcount = dev([count], torch.int32)
            _abi.check(s.L.lrl_sim_observe_idx_dev(s.h, vp(dsome), i32(9), vp(dcount), flags, stream()))
            check(some[:used], f"device count {count} of 9")
        sentinel()
        dcount = dev([0], torch.int32)
        _abi.check(s.L.lrl_sim_observe_idx_dev(s.h, vp(dsome), i32(9), vp(dcount), flags, stream()))
        check(some[:0], "device count 0")


# =================================================================================================================
# Counter-RNG kernels
# =================================================================================================================
RANGES = dict(fr=(0.05, 4.5), rr=(0.0, 1.0), pr=(-1.0, 3.0), cr=(-0.1, 0.1))
DR_FIELDS = (_abi.T_PAYLOAD, _abi.T_COM_DISPLACEMENT, _abi.T_FRICTION, _abi.T_RESTITUTION)  # bits 0, 1, 2, 3


def _randomize(s, which, r=RANGES):
    arr = lambda x: (f32c * 2)(*x)
    _abi.check(s.L.lrl_sim_randomize(s.h, arr(r["fr"]), arr(r["rr"]), arr(r["pr"]), arr(r["cr"]), u32c(which),
                                     stream()))
    sync()
    return [npy(s.t(tid)).copy() for tid in DR_FIELDS]


def _randomize_ref(n, offset, seed, r=RANGES):
    rows = [ar.randomize_draws(offset + e, seed, r["fr"], r["rr"], r["pr"], r["cr"]) for e in range(n)]
    return [np.array([x[0] for x in rows], F32), np.stack([x[1] for x in rows]).astype(F32),
            np.array([x[2] for x in rows], F32), np.array([x[3] for x in rows], F32)]


def test_randomize_matches_philox():
    n, seed = 67, 0x1234567089ABCDEF
    want = _randomize_ref(n, 0, seed)
    assert all(len(np.unique(w)) > n // 2 for w in want)
    with mc_sim(n, seed=seed) as s:
        for which in (0, 1, 2, 4, 8, 15):
            for tid in DR_FIELDS:
                s.t(tid).fill_(-99.0)
            got = _randomize(s, which)
            for bit, (g, w) in enumerate(zip(got, want)):
                if which >> bit & 1:
                    same(g, w, f"which {which}: field {bit}")
                else:
                    assert (g == -99.0).all(), f"which {which}: field {bit} was not selected"
        # a degenerate range gives its end exactly
        flat = dict(fr=(0.7, 0.7), rr=(0.25, 0.25), pr=(-1.5, -1.5), cr=(0.1, 0.1))
        for g, v in zip(_randomize(s, 15, flat), (-1.5, 0.1, 0.7, 0.25)):
            assert (g == F32(v)).all()
    with mc_sim(n, seed=seed + 1) as s:
        other = _randomize(s, 15)
    same(other[0], _randomize_ref(n, 0, seed + 1)[0], "second seed")
    assert all((a != b).mean() > 0.9 for a, b in zip(other, want))


RESET_OVER = {"domain_rand.randomize_motor_strength": True, "domain_rand.motor_strength_range": [0.9, 1.1],
              "domain_rand.randomize_Kp_factor": True, "domain_rand.Kp_factor_range": [0.8, 1.3],
              "domain_rand.randomize_Kd_factor": True, "domain_rand.Kd_factor_range": [0.5, 1.5]}
XY_LO, XY_HI, X_OFF, Y_OFF = -0.5, 0.75, 0.25, -0.125
RESET_STATE = (_abi.T_ROOT_STATE, _abi.T_DOF_POS, _abi.T_DOF_VEL, _abi.T_LAST_ACTIONS, _abi.T_LAST_DOF_VEL,
               _abi.T_MOTOR_STRENGTH, _abi.T_KP_FACTOR, _abi.T_KD_FACTOR, _abi.T_FEET_AIR_TIME,
               _abi.T_EPISODE_LENGTH, _abi.T_RESET)


def _fill_reset_state(s, rng):
    for tid in RESET_STATE:
        t = s.t(tid)
        if t.dtype == torch.float32:
            t.copy_(dev(rng.uniform(1, 9, tuple(t.shape))))
        elif t.dtype == torch.int32:
            t.copy_(dev(rng.integers(1, 99, tuple(t.shape)), torch.int32))
        else:
            t.zero_()
    s.t(_abi.T_ENV_ORIGINS).copy_(dev(rng.uniform(-30, 30, (s.n, 3))))
    return {tid: npy(s.t(tid)).copy() for tid in RESET_STATE + (_abi.T_ENV_ORIGINS,)}


def _reset_ref(before, P, offset, seed, ids, counts, mode):
    """The state after reset_kernel's counter-RNG reset of ``ids`` (float32, the reference's operation order)."""
    f = F32
    after = {k: v.copy() for k, v in before.items()}
    span = lambda r: f(float(r[1]) - float(r[0]))  # the python-float difference, rounded once
    dr = ((RESET_OVER["domain_rand.motor_strength_range"], _abi.T_MOTOR_STRENGTH),
          (RESET_OVER["domain_rand.Kp_factor_range"], _abi.T_KP_FACTOR),
          (RESET_OVER["domain_rand.Kd_factor_range"], _abi.T_KD_FACTOR))
    init = np.array(P.base_init_state[:], f)
    for e in ids:
        u = ar.reset_uniforms(offset + e, counts[e], seed)
        for k, (r, tid) in enumerate(dr):
            after[tid][e, :] = ar.draw32(u[k], span(r), f(r[0]))
        after[_abi.T_DOF_POS][e] = np.array(P.default_dof_pos[:], f)
        for tid in (_abi.T_DOF_VEL, _abi.T_LAST_ACTIONS, _abi.T_LAST_DOF_VEL, _abi.T_FEET_AIR_TIME):
            after[tid][e] = 0
        after[_abi.T_EPISODE_LENGTH][e] = 0
        after[_abi.T_RESET][e] = 1
        if mode != 0:
            root = init.copy()
            root[:3] = init[:3] + before[_abi.T_ENV_ORIGINS][e]
            if mode == 2:
                for c, off in ((0, X_OFF), (1, Y_OFF)):
                    root[c] = f(root[c] + ar.draw32(u[3 + c], f(XY_HI - XY_LO), f(XY_LO))) + f(off)
            after[_abi.T_ROOT_STATE][e] = root
    return after


def _reset(s, ids, mode, dcount=None):
    d = dev(ids, torch.int32)
    xy = (f32c(XY_LO), f32c(XY_HI - XY_LO), f32c(X_OFF), f32c(Y_OFF))
    if dcount is None:
        _abi.check(s.L.lrl_sim_reset_idx_ex(s.h, vp(d), i32(len(ids)), i32(mode), *xy, u32c(0), stream()))
    else:
        dc = dev([dcount], torch.int32)
        _abi.check(s.L.lrl_sim_reset_idx_dev(s.h, vp(d), i32(len(ids)), vp(dc), i32(mode), *xy, stream()))
    sync()
    return {tid: npy(s.t(tid)).copy() for tid in RESET_STATE + (_abi.T_ENV_ORIGINS,)}


def _same_state(got, want, what):
    for tid in want:
        same(got[tid], want[tid], f"{what}: tensor {tid}")


def test_reset_draws_match_philox():
    n, seed = 67, 77
    rng = np.random.default_rng(8)
    _, _, M, P = make("mc", **RESET_OVER)
    assert P.randomize_motor_strength and P.randomize_kp and P.randomize_kd
    perm = rng.permutation(n)
    first, second, third = perm[:20], perm[20:35], perm[35:45]  # disjoint, unsorted, each id once
    counts = np.zeros(n, np.int64)
    with sim_of(M, P, n, seed=seed) as s:
        state = _fill_reset_state(s, rng)
        wants = []
        for ids, mode, what in ((first, 2, "first set, counter 0"), (first, 2, "first set, counter 1"),
                                (second, 2, "second set, counter 0"), (third, 1, "root mode 1"),
                                (first, 0, "root mode 0 leaves the root")):
            want = _reset_ref(state, P, 0, seed, ids, counts, mode)
            wants.append(want)
            # refill what the reset overwrote so that every call starts from distinct values
            for tid in RESET_STATE:
                s.t(tid).copy_(dev(state[tid], s.t(tid).dtype))
            _same_state(_reset(s, ids, mode), want, what)
            counts[ids] += 1
        for tid in (_abi.T_MOTOR_STRENGTH, _abi.T_KP_FACTOR, _abi.T_KD_FACTOR, _abi.T_ROOT_STATE):
            assert (wants[0][tid][first, 0] != wants[1][tid][first, 0]).all()  # counter 1: new draws
        same(wants[4][_abi.T_ROOT_STATE], state[_abi.T_ROOT_STATE], "root mode 0")
        # a device count below the id count: only the first ids reset
        ids = perm[45:55]
        for tid in RESET_STATE:
            s.t(tid).copy_(dev(state[tid], s.t(tid).dtype))
        want = _reset_ref(state, P, 0, seed, ids[:4], counts, 2)
        _same_state(_reset(s, ids, 2, dcount=4), want, "device count 4 of 10")
        counts[ids[:4]] += 1
        want = _reset_ref(want, P, 0, seed, ids, counts, 2)
        _same_state(_reset(s, ids, 2, dcount=50), want, "device count 50 of 10 (clamped)")


TORIG_ROWS = TORIG_COLS = 4


def _terrain_curriculum(s, ids, levels, types, torig, half, T, max_level, dcount=None):
    d = dev(ids, torch.int32)
    args = (vp(levels), vp(types))
    tail = (vp(torig), i32(TORIG_ROWS), i32(TORIG_COLS), f32c(half), f32c(T), i32(max_level), stream())
    if dcount is None:
        _abi.check(s.L.lrl_sim_terrain_curriculum(s.h, vp(d), i32(len(ids)), *args, None, *tail))
    else:
        dc = dev([dcount], torch.int32)
        _abi.check(s.L.lrl_sim_terrain_curriculum_dev(s.h, vp(d), i32(len(ids)), vp(dc), *args, *tail))
    sync()


def test_terrain_curriculum_edges_and_draws():
    n, seed, max_level = 67, 2024, 4
    rng = np.random.default_rng(9)
    torig0 = rng.uniform(-50, 50, (TORIG_ROWS, TORIG_COLS, 3)).astype(F32)
    below5, above2 = float(np.nextafter(F32(5), F32(0))), float(np.nextafter(F32(2), F32(3)))
    with rough_sim(n, seed=seed) as s:
        torig = dev(torig0)
        root, origins, commands = s.t(_abi.T_ROOT_STATE), s.t(_abi.T_ENV_ORIGINS), s.t(_abi.T_COMMANDS)
        org = np.zeros((n, 3), F32)
        org[:, 0:2] = rng.integers(-40, 40, (n, 2))
        pos = org.copy()
        pos[:, 0:2] += (3, 4)  # distance 5, exactly
        types0 = rng.integers(0, TORIG_COLS, n)

        def run(levels0, cmd, half, T, counter, ids=None, dcount=None):
            """One launch over ``ids`` (all envs, shuffled) from levels0; returns (levels, origins) after it."""
            ids = rng.permutation(n) if ids is None else ids
            root[:, 0:3] = dev(pos)
            origins.copy_(dev(org))
            c = np.zeros((n, 4), F32)
            c[:, 0:2] = cmd
            commands.copy_(dev(c))
            levels, types = dev(levels0, torch.int64), dev(types0, torch.int64)
            _abi.check(s.L.lrl_sim_set_step_counter(s.h, i64(counter)))
            _terrain_curriculum(s, ids, levels, types, torig, half, T, max_level, dcount)
            same(npy(types), types0.astype(np.int64), "types untouched")
            return npy(levels), npy(origins)

        def expect(levels0, move, counter, ids=None):
            lv = np.asarray(levels0, np.int64).copy()
            ids = np.arange(n) if ids is None else ids
            for e in ids:
                x = lv[e] + move
                if x >= max_level:
                    x = ar.terrain_level_draw(e, counter, seed, max_level)
                lv[e] = max(x, 0)
            o = org.copy()
            o[ids] = torig0[lv[ids], types0[ids]]
            return lv, o

        mid = rng.integers(1, max_level - 1, n)  # levels 1..2: a move of one stays inside [0, max_level)
        cases = [  # (what, levels, command xy, half, T, step counter, expected move)
            ("distance = half stays (strictly greater moves up)", mid, (0, 0), 5.0, 2.0, 10, 0),
            ("half one ulp below the distance moves up", mid, (0, 0), below5, 2.0, 10, +1),
            ("distance = (|cmd| T) / 2 stays (strictly less moves down)", mid, (3, 4), 100.0, 2.0, 10, 0),
            ("distance just under (|cmd| T) / 2 moves down", mid, (3, 4), 100.0, above2, 10, -1),
            ("up wins when both hold", mid, (6, 8), below5, 2.0, 10, +1),
            ("down", mid, (6, 8), 100.0, 2.0, 10, -1),
            ("the level clamps at 0", np.zeros(n, np.int64), (6, 8), 100.0, 2.0, 10, -1),
            ("past the top: a uniform draw, counter below 2^32", np.full(n, max_level - 1), (0, 0), 1.0, 2.0,
             123456789, +1),
            ("past the top: the counter's high word enters the key", np.full(n, max_level - 1), (0, 0), 1.0, 2.0,
             (5 << 32) + 123456789, +1),
        ]
        drawn = []
        for what, levels0, cmd, half, T, counter, move in cases:
            got_l, got_o = run(levels0, cmd, half, T, counter)
            want_l, want_o = expect(levels0, move, counter)
            same(got_l, want_l, f"{what}: levels")
            same(got_o, want_o, f"{what}: origins = terrain_origins[level, type]")
            if "draw" in what or "key" in what:
                drawn.append(got_l)
        assert all(set(np.unique(d)) == set(range(max_level)) for d in drawn)  # uniform over [0, max_level)
        assert (drawn[0] != drawn[1]).any()
        # a device count below the id count: only the first ids move
        ids = rng.permutation(n)[:30]
        got_l, got_o = run(mid, (6, 8), 100.0, 2.0, 10, ids=ids, dcount=12)
        want_l, want_o = expect(mid, -1, 10, ids=ids[:12])
        same(got_l, want_l, "device count 12 of 30: levels")
        same(got_o, want_o, "device count 12 of 30: origins")
        got_l, _ = run(np.full(n, max_level - 1), (0, 0), 1.0, 2.0, 99, ids=ids, dcount=1000)
        same(got_l, expect(np.full(n, max_level - 1), +1, 99, ids=ids)[0], "device count draws, clamped count")


def test_sharded_sims_draw_what_one_sim_draws():
    """DESIGN 6 at kernel level: envs 0..60 of a sim at env_offset 67 get, env for env, what envs 67..127 of a
    128-env sim at offset 0 get from the same seed: the randomised properties, the reset draws, the terrain levels."""
    seed, max_level = 31337, 4
    rng = np.random.default_rng(10)
    torig0 = rng.uniform(-50, 50, (TORIG_ROWS, TORIG_COLS, 3)).astype(F32)
    cfg, rob, M, P = make_rough(**RESET_OVER)
    out = {}
    for name, n, offset in (("whole", 128, 0), ("shard", 61, 67)):
        with sim_of(M, P, n, offset=offset, seed=seed) as s:
            got = _randomize(s, 15)
            want = _randomize_ref(n, offset, seed)
            for g, w in zip(got, want):
                same(g, w, f"{name}: randomised field")
            s.t(_abi.T_ENV_ORIGINS).zero_()
            resets = []
            for _ in range(2):  # reset counters 0 and 1
                st = _reset(s, np.random.default_rng(n).permutation(n), 2)
                resets += [st[_abi.T_MOTOR_STRENGTH], st[_abi.T_KP_FACTOR], st[_abi.T_KD_FACTOR],
                           st[_abi.T_ROOT_STATE]]
            levels = dev(np.full(n, max_level - 1), torch.int64)
            types = dev(np.zeros(n), torch.int64)
            s.t(_abi.T_ROOT_STATE)[:, 0:2] = 7.0  # far from the origins: every env moves up, past the top
            _abi.check(s.L.lrl_sim_set_step_counter(s.h, i64((1 << 32) + 5)))
            _terrain_curriculum(s, np.arange(n), levels, types, dev(torig0), 1.0, 2.0, max_level)
            out[name] = got + resets + [npy(levels)]
    for k, (a, b) in enumerate(zip(out["whole"], out["shard"])):
        same(b, a[67:128], f"field {k} of the shard against envs 67..127 of the whole")
        assert len(np.unique(b.reshape(len(b), -1)[:, 0])) > (3 if k == len(out["whole"]) - 1 else 30)


# =================================================================================================================
# Indexed setters and apply_commands_kernel
# =================================================================================================================
def _unique(rng, shape):
    return rng.permutation(int(np.prod(shape))).reshape(shape).astype(F32) + F32(0.5)


def test_indexed_setters():
    n = 67
    rng = np.random.default_rng(12)
    with mc_sim(n) as s:
        root, pos, vel = s.t(_abi.T_ROOT_STATE), s.t(_abi.T_DOF_POS), s.t(_abi.T_DOF_VEL)
        r0, p0, v0 = _unique(rng, (n, 13)), _unique(rng, (n, 12)), _unique(rng, (n, 12))
        root.copy_(dev(r0))
        pos.copy_(dev(p0))
        vel.copy_(dev(v0))
        src_r, src_p, src_v = -_unique(rng, (n, 13)), -_unique(rng, (n, 12)), -_unique(rng, (n, 12))
        dr, dp, dv = dev(src_r), dev(src_p), dev(src_v)
        ids = rng.permutation(n)[:23].astype(np.int32)
        dids = dev(ids, torch.int32)
        # no ids: nothing moves
        _abi.check(s.L.lrl_sim_set_root_state_indexed(s.h, vp(dr), None, i32(0), stream()))
        _abi.check(s.L.lrl_sim_set_dof_state_indexed(s.h, vp(dp), vp(dv), vp(dids), i32(0), stream()))
        sync()
        same(npy(root), r0, "root after n = 0")
        same(npy(pos), p0, "dof_pos after n = 0")
        same(npy(vel), v0, "dof_vel after n = 0")
        _abi.check(s.L.lrl_sim_set_root_state_indexed(s.h, vp(dr), vp(dids), i32(len(ids)), stream()))
        sync()
        want = r0.copy()
        want[ids] = src_r[ids]
        same(npy(root), want, "set_root: the source's rows at the ids, every other row unchanged")
        same(npy(pos), p0, "set_root leaves dof_pos")
        _abi.check(s.L.lrl_sim_set_dof_state_indexed(s.h, vp(dp), vp(dv), vp(dids), i32(len(ids)), stream()))
        sync()
        wp, wv = p0.copy(), v0.copy()
        wp[ids], wv[ids] = src_p[ids], src_v[ids]
        same(npy(pos), wp, "set_dof: positions")
        same(npy(vel), wv, "set_dof: velocities")
        same(npy(root), want, "set_dof leaves the root")
        assert s.L.lrl_sim_set_root_state_indexed(s.h, None, vp(dids), i32(3), stream()) != 0
        assert s.L.lrl_sim_set_dof_state_indexed(s.h, vp(dp), None, vp(dids), i32(3), stream()) != 0


def test_apply_commands():
    n = 67
    rng = np.random.default_rng(13)
    with mc_sim(n) as s:
        commands, sums = s.t(_abi.T_COMMANDS), s.t(_abi.T_COMMAND_SUMS)
        ncs = sums.shape[0]
        c0, s0 = _unique(rng, (n, 4)), _unique(rng, (ncs, n))
        bins0 = _unique(rng, (n,))
        bins_in = dev(bins0)

        def run(k, nbins, with_bins=True):
            commands.copy_(dev(c0))
            sums.copy_(dev(s0))
            ids = rng.permutation(n)[:k].astype(np.int32)
            cmds = -_unique(rng, (max(k, 1), 3))
            bins_out = torch.full((n + 5,), -8.0, device=DEV)
            dids, dcmds = dev(ids, torch.int32), dev(cmds)
            rc = s.L.lrl_sim_apply_commands(s.h, vp(dids) if k else None, i32(k), vp(dcmds) if k else None,
                                            vp(bins_in) if with_bins else None, vp(bins_out) if with_bins else None,
                                            i32(nbins), stream())
            sync()
            return rc, ids, cmds[:k], npy(bins_out)

        def check(k, nbins, with_bins=True):
            rc, ids, cmds, bins = run(k, nbins, with_bins)
            what = f"{k} ids, {nbins} bins" + ("" if with_bins else " (null)")
            assert rc == 0, what
            wc, ws = c0.copy(), s0.copy()
            wc[ids, :3] = cmds
            ws[:, ids] = 0.0
            same(npy(commands), wc, f"{what}: commands[ids, :3], column 3 and the other envs unchanged")
            same(npy(sums), ws, f"{what}: command sums zero at the ids, unchanged elsewhere")
            wb = np.full(n + 5, -8.0, F32)
            if with_bins:
                wb[:nbins] = bins0[:nbins]
            same(bins, wb, f"{what}: bins")

        for k, nbins in ((20, 0), (3, 5), (20, 5), (20, n), (n, n), (1, n)):
            check(k, nbins)
        check(0, 5)              # bins only
        check(0, n)
        check(20, 5, with_bins=False)
        check(0, 0, with_bins=False)  # nothing to do
        rc, _, _, bins = run(20, n + 1)
        assert rc != 0
        same(npy(commands), c0, "refused: commands")
        same(npy(sums), s0, "refused: sums")
        assert (bins == -8.0).all()
