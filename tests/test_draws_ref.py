"""CPU pins of the draw helpers of tests/aux_ref.py (observation noise, pushes, the per-step redraw, policy noise) that
tests/test_draws_gpu.py and tests/test_policy_draws_gpu.py hold the kernels to:

* the vectorised Philox equals the integer one (which test_aux_ref.py pins on Random123's known answers);
* the Box-Muller reference is a standard normal per action, the two members of a pair uncorrelated;
* the key whose first uniform is exactly 0 (the clamp at 1e-7) is recomputed here;
* a float32 evaluation of the Box-Muller formula stays within a quarter of the bar the kernels are given;
* the CPU oracle without injection gives the bits it gives with the helpers' uniforms injected: the two-run design of
  the GPU test.  The oracle includes include/lrl_philox.h as the kernels do, so this confirms the helpers' counter
  layout (env id, counter words, stream, block, word) and nothing beyond it.
"""
import numpy as np
import pytest

import aux_ref as ar
import draws_cases as dc
from helpers import make, make_rough, same
from lrl import _abi
from oracle import oracle
from test_aux_ref import PHILOX_KAT

F32 = np.float32


# ---------------------------------------------------------------------------------------------- the vectorised Philox
def test_vectorised_philox_equals_the_integer_one():
    for ctr, key, want in PHILOX_KAT:
        got = ar.philox_v(*ctr, key[0] | key[1] << 32)
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4, 200), dtype=np.uint64)
    c[:, :4] = [[0, 0xFFFFFFFF, 0, 0xFFFFFFFF]] * 4  # the ends of the word range
    for seed in (0, 11, dc.SEED, 2 ** 64 - 1):
        got = ar.philox_v(c[0], c[1], c[2], c[3], seed)
        for i in range(c.shape[1]):
            assert tuple(int(x) for x in got[i]) == ar.philox(*(int(x) for x in c[:, i]), seed), (seed, i)
    # broadcasting: a column of rows against a row of blocks
    got = ar.philox_v(np.arange(5)[:, None], 7, 9, np.arange(3)[None, :], 11)
    assert got.shape == (5, 3, 4)
    assert tuple(int(x) for x in got[4, 2]) == ar.philox(4, 7, 9, 2, 11)
    x = rng.integers(0, 2 ** 32, 100, dtype=np.uint64).astype(np.uint32)
    x[:3] = [0, 0xFF, 0xFFFFFFFF]
    same(ar.u01_v(x), np.array([ar.u01(v) for v in x], F32), "u01_v")


# ---------------------------------------------------------------------------------------------- the step's helpers
def test_step_helpers_take_the_documented_words():
    genv, seed = 1003, dc.SEED
    for counter in (1, dc.WRAP + 1):
        lo, hi = counter & ar.M32, counter >> 32
        for NO in (42, 45, 48, 51):
            u = ar.obs_noise_uniforms(genv, counter, seed, NO)
            assert u.shape == (NO,) and u.dtype == F32
            for i in (0, 3, 4, NO - 2, NO - 1):
                assert u[i] == ar.u01(ar.philox(genv, lo, (ar.RNG_OBS_NOISE << 16) ^ hi, i >> 2, seed)[i & 3])
        r = ar.philox(genv, lo, (ar.RNG_PUSH << 16) ^ hi, 0, seed)
        same(ar.push_uniforms(genv, counter, seed), np.array([ar.u01(r[0]), ar.u01(r[1])], F32), "push")
        r = ar.philox(genv, lo, (ar.RNG_DR << 16) ^ hi, 0, seed)
        for ms in (0, 1):
            for kp in (0, 1):
                for kd in (0, 1):
                    u, word = ar.dr_uniforms(genv, counter, seed, ms, kp, kd)
                    on = [i for i, s in enumerate((ms, kp, kd)) if s]
                    assert [int(word[i]) for i in on] == list(range(len(on)))  # a switch that is off takes no word
                    for i in range(3):
                        if i in on:
                            assert u[i] == ar.u01(r[word[i]])
                        else:
                            assert word[i] == -1 and np.isnan(u[i])
    # the counter's high word reaches the key, the env id's high bits do not reach anything
    assert not np.array_equal(ar.obs_noise_uniforms(3, 5, seed, 8), ar.obs_noise_uniforms(3, 5 + (1 << 32), seed, 8))
    same(ar.obs_noise_uniforms(3 + (1 << 32), 5, seed, 8), ar.obs_noise_uniforms(3, 5, seed, 8), "env id mod 2^32")


# ---------------------------------------------------------------------------------------------- policy noise
def test_policy_normals_rows_equals_policy_normals():
    for seed, counter, ro, n in dc.act_keys():
        rows = ro + np.unique(np.concatenate([np.arange(min(n, 3)), [n - 1]]))
        for na in (3, 12):
            e, rad = ar.policy_normals_rows(rows, counter, seed, na)
            for i, g in enumerate(rows):
                e1, rad1 = ar.policy_normals(int(g), counter, seed, na)
                assert np.array_equal(e[i], e1) and np.array_equal(rad[i], rad1), (seed, counter, g, na)


def test_policy_normals_are_standard_normal():
    """16384 rows x 12 actions (196608 draws): per action the mean within 4 / sqrt(n) of 0 and the variance within
    4 sqrt(2 / n) of 1; the correlation of the two members of each pair (one Philox block, cos and sin of one angle)
    within 4 / sqrt(n) of 0."""
    n, na = 16384, 12
    e, rad = ar.policy_normals_rows(1000 + np.arange(n), dc.ACT_COUNTERS[1], dc.ACT_SEED, na)
    assert e.shape == (n, na) and np.isfinite(e).all()
    se = 1.0 / np.sqrt(n)
    assert np.abs(e.mean(0)).max() <= 4 * se, e.mean(0)
    assert np.abs(e.var(0) - 1.0).max() <= 4 * np.sqrt(2.0) * se, e.var(0)
    for p in range(na // 2):
        c = np.corrcoef(e[:, 2 * p], e[:, 2 * p + 1])[0, 1]
        assert abs(c) <= 4 * se, (p, c)
        assert np.array_equal(rad[:, 2 * p], rad[:, 2 * p + 1])
        np.testing.assert_allclose(e[:, 2 * p] ** 2 + e[:, 2 * p + 1] ** 2, rad[:, 2 * p] ** 2, rtol=1e-12)
    # the 8192-row case of the GPU test: its reference itself meets that test's bars
    e, _ = ar.policy_normals_rows(np.arange(dc.STATS_N), dc.STATS_COUNTER, dc.ACT_SEED, na)
    se = 1.0 / np.sqrt(dc.STATS_N)
    assert np.abs(e.mean(0)).max() <= 4 * se and np.abs(e.var(0) - 1.0).max() <= 4 * np.sqrt(2.0) * se
    e3, _ = ar.policy_normals_rows(np.arange(dc.STATS_N), dc.STATS_COUNTER, dc.ACT_SEED, 3)
    assert np.array_equal(e3, e[:, :3])  # an odd action count leaves the last pair half used


def test_the_clamped_key():
    """Global row 2473292 at seed 11, counter 3: block 1 (actions 2 and 3) has a first word below 2^8, so u01 is 0
    exactly and the kernels' clamp at 1e-7f decides the radius."""
    w = ar.philox(dc.CLAMP_ROW, dc.CLAMP_COUNTER, ar.RNG_POLICY << 16, dc.CLAMP_BLOCK, dc.CLAMP_SEED)
    assert w[0] == 0x56 and w[1] == 0x39178BDD
    assert ar.u01(w[0]) == 0.0 and ar.u01(w[1]) == F32(0.22301549)
    e, rad = ar.policy_normals(dc.CLAMP_ROW, dc.CLAMP_COUNTER, dc.CLAMP_SEED, 12)
    assert np.isfinite(e).all()
    want = np.sqrt(-2.0 * np.log(np.float64(F32(1e-7))))
    assert rad[2] == want and rad[3] == want and 5.67 < want < 5.68
    th = np.float64(F32(F32(6.283185307179586) * F32(0.22301549)))
    assert e[2] == want * np.cos(th) and e[3] == want * np.sin(th)
    # the search that found it, over its neighbourhood: the only such block of these rows
    rows = dc.CLAMP_ROW - 5 + np.arange(16)
    w0 = ar.philox_v(rows[:, None], dc.CLAMP_COUNTER, ar.RNG_POLICY << 16, np.arange(6)[None, :], dc.CLAMP_SEED)[..., 0]
    assert np.argwhere(w0 < 256).tolist() == [[5, dc.CLAMP_BLOCK]]


def _box_muller_f32(u1, u2, odd):
    """The kernels' lines in numpy float32, one rounding per operation."""
    u1 = np.maximum(u1.astype(F32), F32(1e-7))
    rad = np.sqrt(F32(-2.0) * np.log(u1))
    th = F32(6.283185307179586) * u2.astype(F32)
    assert rad.dtype == F32 and th.dtype == F32
    return np.where(odd, rad * np.sin(th), rad * np.cos(th)).astype(F32)


def test_float32_box_muller_stays_within_a_quarter_of_the_bar():
    """The bar of the GPU test, 8 x 2^-24 rad + 4 x 2^-24 (|mu| / sd + |e|), is not taken from the kernels: a float32
    numpy evaluation of the same formula (mu = 0: the draw alone) uses at most a quarter of it on every key the GPU
    tests draw with."""
    worst = 0.0
    na = 12
    j = np.arange(na)
    for seed, counter, ro, n in dc.act_keys():
        c1, c2 = ar.step_key(ar.RNG_POLICY, counter)
        w = ar.philox_v((ro + np.arange(n))[:, None], c1, c2, (j >> 1)[None, :], seed)
        u1, u2 = ar.u01_v(w[..., 0]), ar.u01_v(w[..., 1])
        odd = ((j & 1) == 1)[None, :]
        e_ref, rad = ar.box_muller(u1, u2, odd)
        e32 = _box_muller_f32(u1, u2, odd).astype(np.float64)
        ratio = np.abs(e32 - e_ref) / ar.policy_noise_bound(rad, e_ref)
        worst = max(worst, float(ratio.max()))
    print(f"float32 numpy Box-Muller: worst |e32 - e64| / bar = {worst:.3f}")
    assert worst <= 0.25, worst


# ---------------------------------------------------------------------------------------------- the oracle, two runs
def _oracle_state(M, P, n, rng, xy):
    st = oracle.make_state(n, M.num_bodies, P.num_obs, P.num_history, P.num_sum_keys + 1, P.num_sum_keys + 5,
                           num_height_points=P.num_height_points)
    st["root"][:, 0:2] = rng.uniform(xy[0], xy[1], (n, 2))
    st["root"][:, 2] = rng.uniform(0.3, 0.6, n)
    ang = rng.normal(size=(n, 3)) * 0.2
    th = np.linalg.norm(ang, axis=1, keepdims=True)
    st["root"][:, 3:7] = np.concatenate([ang / th * np.sin(th / 2), np.cos(th / 2)], 1)
    st["root"][:, 7:10] = rng.normal(size=(n, 3)) * 0.5
    st["root"][:, 10:13] = rng.normal(size=(n, 3))
    st["dof_pos"][:] = np.array(P.default_dof_pos[:], F32)[None] + rng.normal(size=(n, 12)) * 0.2
    st["dof_vel"][:] = rng.normal(size=(n, 12))
    st["commands"][:] = rng.uniform(-1, 1, (n, 4))
    st["friction"][:] = rng.uniform(0.1, 4, n)
    st["restitution"][:] = rng.uniform(0, 1, n)
    for k in ("motor_strength", "kp", "kd"):  # values no redraw gives: an env not due keeps them visibly
        st[k][:] = np.repeat(rng.uniform(3.0, 4.0, (n, 1)), 12, 1)
    st["hist"][:] = rng.uniform(-1, 1, st["hist"].shape)
    st["episode_length"][:] = dc.EPLEN_POOL[np.arange(n) % len(dc.EPLEN_POOL)]
    return st


@pytest.mark.parametrize("kind", ["mc plane", "go1 rough"])
def test_oracle_draws_what_the_helpers_inject(kind):
    n, offset, counter = 9, 1000, dc.WRAP + 1  # (the oracle takes the counter after the increment)
    if kind == "mc plane":
        _, _, M, P0 = make("mc")
    else:
        _, _, M, P0 = make_rough()
        G = 120
        hs, vs = P0.horizontal_scale, P0.vertical_scale
        samples = dc.gentle_heights(G, hs, vs)
        i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
        v = np.stack([i * hs - P0.border_size, j * hs - P0.border_size, samples * np.float64(vs)], -1)
        oracle.set_terrain(v, samples.astype(F32) * F32(vs))
    P = dc.visible_params(P0)
    assert P.num_obs == (42 if kind == "mc plane" else 229) and counter >> 32 == 6
    blocks = dc.blocks_of(P, None, n, n)
    act = np.random.default_rng(3).uniform(-1.5, 1.5, (n, 12)).astype(F32)
    flags = _abi.STEP_PHYSICS | _abi.STEP_HISTORY
    start = _oracle_state(M, P, n, np.random.default_rng(17), (2.0, 6.0))
    redraw, push = dc.due(blocks, P.rand_interval, start["episode_length"])
    assert 0 < redraw.sum() < n and 0 < push.sum() < n
    noise, dr_u, word, push_u = dc.step_uniforms(blocks, P.num_obs, offset, counter, dc.SEED)
    a = {k: v.copy() for k, v in start.items()}
    b = {k: v.copy() for k, v in start.items()}
    oracle.env_step(M, P, a, act, flags, seed=dc.SEED, env_offset=offset, common_step_counter=counter)
    oracle.env_step(M, P, b, act, flags | _abi.STEP_INJECT_UNIFORM, seed=dc.SEED, env_offset=offset,
                    common_step_counter=counter, noise_u=noise, dr_u=dc.injected_ms(dr_u), push_u=push_u)
    assert np.isfinite(a["obs"]).all()
    # Kp and Kd have no injection (both runs draw them): compared with the helper's words directly
    for k, col in (("kp", 1), ("kd", 2)):
        lo = getattr(P, k + "_range")[0]
        want = start[k].copy()
        want[redraw] = ar.draw32(dr_u[redraw, col], P.dr_span[col], lo)[:, None]
        same(a[k], want, f"{kind}: {k} of run A")
        assert np.array_equal(word[:, col], np.full(n, col))
    for k in oracle.ENV_FIELDS:
        same(a[k], b[k], f"{kind}: {k}")
    # the draws were there to be seen
    assert (a["obs"] != start["obs"]).all() and np.abs(a["obs"]).max() < P.clip_obs
    assert (a["motor_strength"][redraw] != start["motor_strength"][redraw]).all()
    same(a["motor_strength"][~redraw], start["motor_strength"][~redraw], "motor strength of envs not due")
    want = ar.draw32(push_u[push], P.push_span, P.push_lo)
    same(a["root"][push, 7:9], want, "pushed velocity")
    # another counter, env offset or seed: other draws
    for kw in (dict(common_step_counter=counter + 1), dict(env_offset=offset + 1), dict(seed=dc.SEED ^ (1 << 40))):
        c = {k: v.copy() for k, v in start.items()}
        oracle.env_step(M, P, c, act, flags, **dict(dict(seed=dc.SEED, env_offset=offset,
                                                         common_step_counter=counter), **kw))
        assert (c["obs"] != a["obs"]).mean() > 0.95, kw
