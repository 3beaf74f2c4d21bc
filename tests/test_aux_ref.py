"""CPU pins of tests/aux_ref.py on facts from outside this repository's kernels: the Random123 known answers for
Philox4x32-10, closed-form rotations, the joint_xyz sums of the robot tables, and central finite differences of the
position / rotation function for the velocities of ``fk``.
"""
import numpy as np
import pytest

import aux_ref as ar
from helpers import make


# Random123 kat_vectors, philox4x32 10 rounds: (counter words, key words) -> output words
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    assert ar.philox(*ctr, key[0] | key[1] << 32) == want


def test_philox_header_matches_restatement():
    """include/lrl_philox.h compiled for the host gives the restatement's words (the header is what the kernels
    include); skipped only where no C compiler is installed."""
    import ctypes
    import os
    import shutil
    import subprocess
    import tempfile
    cc = next((c for c in map(shutil.which, ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang")) if c), None)
    if cc is None:
        pytest.skip("no C compiler")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "p.c")
        with open(src, "w") as f:
            f.write('#include "lrl_philox.h"\n'
                    "void px(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint64_t s, uint32_t* o) {\n"
                    "  lrl_u32x4 r = lrl_philox(a, b, c, d, s); for (int i = 0; i < 4; ++i) o[i] = r.v[i]; }\n"
                    "float pu(uint32_t x) { return lrl_u01(x); }\n")
        so = os.path.join(d, "p.so")
        subprocess.run([cc, "-O1", "-shared", "-fPIC", "-I", inc, src, "-o", so], check=True)
        L = ctypes.CDLL(so)
        L.pu.restype = ctypes.c_float
        rng = np.random.default_rng(0)
        for _ in range(50):
            c = [int(x) for x in rng.integers(0, 2 ** 32, 4)]
            seed = int(rng.integers(0, 2 ** 63)) * 2 + 1
            out = (ctypes.c_uint32 * 4)()
            L.px(*[ctypes.c_uint32(x) for x in c], ctypes.c_uint64(seed), out)
            assert tuple(out) == ar.philox(*c, seed)
            assert np.float32(L.pu(ctypes.c_uint32(c[0]))) == ar.u01(c[0])


def test_u01_range_and_value():
    assert ar.u01(0) == 0.0 and ar.u01(0xff) == 0.0  # the low 8 bits do not count
    assert ar.u01(0x100) == np.float32(2.0 ** -24)
    top = ar.u01(0xffffffff)
    assert top == np.float32(1.0 - 2.0 ** -24) and top < 1.0 and top.dtype == np.float32
    assert ar.u01(0x80000000) == 0.5


def test_terrain_level_draw_is_the_scaled_word():
    w = ar.philox(5, 7, ar.RNG_TERRAIN << 16, 0, 9)[0]
    assert ar.terrain_level_draw(5, 7, 9, 4) == w * 4 // 2 ** 32
    # the counter's high word enters the key
    assert ar.terrain_level_draw(5, 7 + (3 << 32), 9, 1 << 20) == \
        (ar.philox(5, 7, (ar.RNG_TERRAIN << 16) ^ 3, 0, 9)[0] << 20) >> 32


def test_rotation_conventions():
    s = np.sqrt(0.5)
    Rz = ar.quat_to_mat([0, 0, s, s])  # +90 degrees about z: x -> y
    np.testing.assert_allclose(Rz @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    np.testing.assert_allclose(ar.quat_to_mat([0, 0, 2 * s, 2 * s]), Rz, atol=1e-15)  # normalised first
    np.testing.assert_allclose(ar.axis_angle_mat([0, 0, 1], np.pi / 2), Rz, atol=1e-15)
    np.testing.assert_allclose(ar.axis_angle_mat([1, 0, 0], np.pi / 2) @ [0, 1, 0], [0, 0, 1], atol=1e-15)
    np.testing.assert_allclose(ar.rot_exp(np.array([0, np.pi / 2, 0])) @ [0, 0, 1], [1, 0, 0], atol=1e-15)
    rng = np.random.default_rng(1)
    for _ in range(20):
        q, a = rng.normal(size=4), rng.normal(size=3)
        for R in (ar.quat_to_mat(q), ar.axis_angle_mat(a, rng.uniform(-4, 4))):
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
            assert abs(np.linalg.det(R) - 1) < 1e-14
        # the axis is fixed by its rotation
        np.testing.assert_allclose(ar.axis_angle_mat(a, 1.3) @ a, a, atol=1e-14)


def test_quat_mat_branch():
    assert ar.quat_mat_branch(np.eye(3)) == (0, 3.0)
    for k, q in enumerate(([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0])):  # 180 degrees about x, y, z
        b, margin = ar.quat_mat_branch(ar.quat_to_mat(q))
        assert b == 1 + k and margin == 1.0  # diag (1, -1, -1): trace -1, gap 2 -> the nearer boundary is the trace
    b, margin = ar.quat_mat_branch(np.diag([-0.5, -0.5 + 1e-5, 0.0]) - 0)
    assert b == 3 and abs(margin - 0.5) < 1e-4
    b, margin = ar.quat_mat_branch(np.diag([0.3, 0.3 - 1e-6, -1.0]))
    assert b == 1 and margin < 1e-4


@pytest.mark.parametrize("robot", ["mc", "go1"])
def test_fk_zero_pose_is_the_sum_of_joint_offsets(robot):
    rob = make(robot)[1]
    root = np.zeros(13)
    root[6] = 1.0
    pos, rot, vel, ang = ar.fk(rob, root, np.zeros(3), np.zeros(12), np.zeros(12))
    assert np.array_equal(np.asarray(rob["joint_quat"]).reshape(-1, 4), np.tile([0, 0, 0, 1.0], (12, 1)))
    seen = set()
    for b, (leg, link) in enumerate(zip(rob["body_leg"], rob["body_link"])):
        want = np.zeros(3)
        if leg >= 0:
            want = np.sum(np.asarray(rob["joint_xyz"][leg])[: min(link, 2) + 1], axis=0)
            if link == 3:
                want = want + np.asarray(rob["foot_xyz"][leg])
        np.testing.assert_allclose(pos[b], want, atol=1e-15)
        np.testing.assert_allclose(rot[b], np.eye(3), atol=1e-15)
        seen.add((leg, link))
    assert np.all(vel == 0) and np.all(ang == 0)
    # the feet: Go1 has foot bodies (link 3), Mini Cheetah's feet are its calves
    assert (((0, 3) in seen) == (robot == "go1")) and len(seen) == rob["num_bodies"]


def test_fk_base_velocity_is_about_the_centre_of_mass():
    """A base spinning about its centre of mass (V = 0): the origin, at -R com from it, moves at -W x (R com); with no
    displacement it stands still."""
    rob = make("go1")[1]
    q = np.array([0.3, -0.2, 0.5, 0.81])
    root = np.concatenate([[1.0, 2.0, 3.0], q, [0, 0, 0], [0.0, 0.0, 2.0]])
    com = np.array([0.1, 0.0, 0.0])
    vel = ar.fk(rob, root, com, np.zeros(12), np.zeros(12))[2]
    np.testing.assert_allclose(vel[0], -np.cross([0, 0, 2.0], ar.quat_to_mat(q) @ com), atol=1e-15)
    assert np.all(ar.fk(rob, root, np.zeros(3), np.zeros(12), np.zeros(12))[2][0] == 0)


def _random_model(rob, rng):
    m = dict(rob)
    jq = rng.normal(size=(4, 3, 4))
    ja = rng.normal(size=(4, 3, 3))
    m["joint_quat"] = (jq / np.linalg.norm(jq, axis=-1, keepdims=True)).tolist()
    m["joint_axis"] = (ja / np.linalg.norm(ja, axis=-1, keepdims=True)).tolist()
    return m


@pytest.mark.parametrize("model", ["mc", "go1", "go1_random_joints"])
def test_fk_velocities_match_finite_differences(model):
    """The velocities of ``fk`` against central differences of ``body_frames`` in float64: the base pose advanced along
    (origin velocity, W) and the joints along qd by +-h, h = 1e-5; the angular velocity from the skew part of
    (R(+h) R(-h)^T - I) / 2h.

    The bar is the truncation error of the difference, bounded from the path: every factor of a body's pose is a
    rotation at a constant rate, the rates of its chain sum to at most Om = |W| + sum |qd|, and its origin hangs on
    levers of total length Lv = sum |joint_xyz| + |foot_xyz|; so |x'''| <= Om^3 Lv and the central difference of x is
    off by at most h^2 / 6 Om^3 Lv.  F(t) = R(t) R(-t)^T has F(-t) = F(t)^T, so skew((F(h) - I) / 2h) is half the
    central difference of F, whose third derivative is at most (2 Om)^3: off by at most 2/3 h^2 Om^3 (taken as h^2
    Om^3).  Rounding adds about eps (|x| + Lv) / h and eps / h, taken 8 times over."""
    rng = np.random.default_rng({"mc": 2, "go1": 3, "go1_random_joints": 4}[model])
    rob = make("mc" if model == "mc" else "go1")[1]
    if model == "go1_random_joints":
        rob = _random_model(rob, rng)
    h, eps = 1e-5, np.finfo(np.float64).eps
    Lv = max(sum(np.linalg.norm(x) for x in rob["joint_xyz"][leg]) + np.linalg.norm(rob["foot_xyz"][leg])
             for leg in range(4))
    worst_v = worst_w = 0.0
    for _ in range(12):
        quat = rng.normal(size=4)
        root = np.concatenate([rng.uniform(-3, 3, 3), quat / np.linalg.norm(quat), rng.uniform(-2, 2, 3),
                               rng.uniform(-3, 3, 3)])
        com, q, qd = rng.uniform(-0.1, 0.1, 3), rng.uniform(-2.5, 2.5, 12), rng.uniform(-5, 5, 12)
        pos, rot, vel, ang = ar.fk(rob, root, com, q, qd)
        R = ar.quat_to_mat(root[3:7])
        W = root[10:13]
        v0 = root[7:10] - np.cross(W, R @ com)
        Tp = ar.body_frames(rob, root[0:3] + h * v0, ar.rot_exp(h * W) @ R, q + h * qd)
        Tm = ar.body_frames(rob, root[0:3] - h * v0, ar.rot_exp(-h * W) @ R, q - h * qd)
        np.testing.assert_allclose(ar.body_frames(rob, root[0:3], R, q)[:, :3, 3], pos, atol=1e-15)
        Om = np.linalg.norm(W) + max(np.sum(np.abs(qd[3 * leg: 3 * leg + 3])) for leg in range(4))
        bar_v = h * h / 6 * Om ** 3 * Lv + 8 * eps * (np.abs(pos).max() + Lv) / h
        bar_w = h * h * Om ** 3 + 8 * eps / h
        assert bar_v < 1e-6 and bar_w < 1e-5  # the pin is sharp: conventions are O(1) off when wrong
        fd_v = (Tp[:, :3, 3] - Tm[:, :3, 3]) / (2 * h)
        F = np.einsum("bij,bkj->bik", Tp[:, :3, :3], Tm[:, :3, :3])
        S = (F - np.eye(3)) / (2 * h)
        S = (S - np.swapaxes(S, 1, 2)) / 2
        fd_w = np.stack([S[:, 2, 1], S[:, 0, 2], S[:, 1, 0]], 1)
        ev, ew = np.abs(fd_v - vel).max(), np.abs(fd_w - ang).max()
        assert ev <= bar_v, (ev, bar_v)
        assert ew <= bar_w, (ew, bar_w)
        worst_v, worst_w = max(worst_v, ev / bar_v), max(worst_w, ew / bar_w)
    print(f"{model}: worst error / bar: linear {worst_v:.3f}, angular {worst_w:.3f}")


def test_small_references():
    eplen = np.array([0, 1, 2, 5, 6, 13, 2 ** 31 - 2])
    assert ar.due(eplen, 1).all()
    assert list(ar.due(eplen, 3)) == [False, False, True, True, False, False, False]
    assert list(ar.due(eplen, 7)) == [False, False, False, False, True, True, False]
    assert list(ar.due(eplen, 2 ** 31 - 1)) == [False] * 6 + [True]
    reset = np.array([1, 0, 0, 1, 0, 0, 1], np.uint8)
    assert list(ar.env_list(0, reset, eplen, 3)) == [0, 3, 6]
    assert list(ar.env_list(1, reset, eplen, 3)) == [2, 3]
    assert list(ar.step_code(reset, eplen, 3)) == [1, 0, 2, 3, 0, 0, 1]
    hist = np.arange(12, dtype=np.float32).reshape(2, 6)
    obs = -np.arange(1, 5, dtype=np.float32).reshape(2, 2)
    assert ar.shift_history(hist, obs).tolist() == [[2, 3, 4, 5, -1, -2], [8, 9, 10, 11, -3, -4]]
    assert ar.shift_history(hist[:, :2], obs).tolist() == obs.tolist()  # history 1: nothing is kept
    m, a = ar.row_means(np.array([[1.0, -3.0, 5.0, 100.0]]), [2, 0, 1])
    assert m[0] == 1.0 and a[0] == 3.0
    assert np.isnan(ar.row_means(np.ones((2, 3)), [])[0]).all()
