"""tests/curriculum_ref.py (the numpy reference of the device command curriculum) pinned on the CPU: on the reference
project's recorded vectors, against both host forms of lrl.curriculum, and the coverage conditions of the chains that
tests/test_curriculum_dev_gpu.py plays on the device, evaluated on the reference alone.

The one-bin grid and every grid with a one-point axis: ``np.linspace(lo, hi, 1)`` is ``[lo]``, so
``bin_size = axis[1] - axis[0]`` raises IndexError in the cited code, in ``lrl.curriculum`` and in ``CurriculumRef``
alike (asserted below).  The device descriptor carries ``half`` itself, so the kernel is still defined there; the
chains give those axes a bin size of their own, and on these grids the reference is compared with the native host
functions (which take grid, axes and half as arguments) instead of the Python class that cannot be built.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import curriculum_cases as cc
import curriculum_ref as cr
from helpers import golden, make
from lrl import _abi
from lrl.curriculum import RewardThresholdCurriculum

F32 = np.float32
PRODUCTION = ((-10.0, 10.0, 51), (-0.6, 0.6, 2), (-10.0, 10.0, 51))


@functools.lru_cache(None)
def sim_rows():
    """(number of command-sum rows, the (tracking_lin_vel, tracking_ang_vel) rows) of the Mini Cheetah preset."""
    cfg, _, _, P = make("mc")
    return P.num_sum_keys + 5, (0, 1)  # (lrl/env.py's _track_rows: the keys of the non-zero reward scales)


def test_reference_replays_the_recorded_vectors():
    g = golden("curriculum.npz")
    ref = cr.CurriculumRef(PRODUCTION, 4096, 1, seed=100)
    np.testing.assert_array_equal(ref.grid, g["grid"])
    low, high = np.array([-0.6, -0.6, -1.0]), np.array([0.6, 0.6, 1.0])
    ref.weights[np.logical_and(ref.grid >= low[:, None], ref.grid <= high[:, None]).all(axis=0)] = 1.0
    np.testing.assert_array_equal(ref.weights, g["weights0"])
    cmds, bins = ref.sample(64)
    np.testing.assert_array_equal(bins, g["bins1"])
    np.testing.assert_array_equal(cmds, g["cmds1"])
    ref.update(g["upd_bins"], g["lin"], g["ang"], float(g["lin_thr"]), float(g["ang_thr"]), 0.5)
    np.testing.assert_array_equal(ref.weights, g["weights1"])
    cmds, bins = ref.sample(4096)
    np.testing.assert_array_equal(bins, g["bins2"])
    np.testing.assert_array_equal(cmds, g["cmds2"])


def test_threshold_rule_is_float32():
    """The stated rule against the installed numpy on the recorded dtype (float32 rewards, Python thresholds), and
    what separates it from a float64 comparison: float32(thr) itself."""
    for thr in (cc.LIN_THR, cc.ANG_THR):
        t = F32(thr)
        r = np.array([np.nextafter(t, F32(0)), t, np.nextafter(t, F32(1))], F32)
        assert ((r > thr) == (r > t)).all() and (r > t).tolist() == [False, False, True]
        assert (r.astype(np.float64) > thr).tolist() == [False, True, True]


def _host_pair(ranges, seed):
    a, b = (RewardThresholdCurriculum(seed, x=ranges[0], y=ranges[1], z=ranges[2]) for _ in range(2))
    assert a._native
    b._native = False
    return a, b


def _native_sample(ref_like, key, pos, weights, n):
    L = _abi.lib()
    cmds, bins = np.empty((n, 3)), np.empty(n, np.int64)
    grid = np.ascontiguousarray(ref_like.grid)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = L.lrl_curriculum_sample(p(key), p(pos), p(weights), ref_like.nb, p(grid), p(ref_like.half), n, p(cmds), p(bins))
    assert rc == 0
    return cmds, bins


def _native_update(ref_like, weights, centres, local_range):
    axes = np.ascontiguousarray(np.concatenate(ref_like.axes))
    cen = np.ascontiguousarray(centres, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    nx, ny, nz = ref_like.shape
    _abi.check(_abi.lib().lrl_curriculum_update_weights(p(weights), p(axes), nx, ny, nz, p(cen), len(cen),
                                                        C.c_double(local_range)))


GRID_CASES = [("production", dict(ranges=PRODUCTION))] + list(cc.GRIDS.items())


@pytest.mark.parametrize("gname,g", GRID_CASES, ids=[k for k, _ in GRID_CASES])
def test_reference_matches_both_host_forms(gname, g):
    """Random update / sample sequences: weights, episode rewards, bins, commands and the MT key / position of the
    reference against lrl.curriculum's numpy form and its native form (on a grid with a one-point axis, which the
    class refuses, against the native functions called directly)."""
    rng = np.random.default_rng(list(gname.encode()))
    one_point = any(r[2] == 1 for r in g["ranges"])
    ref = cr.CurriculumRef(g["ranges"], 1, 1, seed=7, bin_sizes=g.get("bin_sizes"))
    nb = ref.nb
    w0 = cc.ladder()[rng.integers(0, 6, nb)]
    w0[rng.integers(0, nb)] = 0.4
    ref.weights[:] = w0
    if one_point:
        with pytest.raises(IndexError):
            RewardThresholdCurriculum(7, x=g["ranges"][0], y=g["ranges"][1], z=g["ranges"][2])
        with pytest.raises(IndexError):
            cr.CurriculumRef(g["ranges"], 1, 1)
        key, pos = ref.mt[0].copy(), np.array([ref.mt[1]], np.int32)
        nat_w = w0.copy()
    else:
        nat, py = _host_pair(g["ranges"], 7)
        for c in (nat, py):
            c.weights[:] = w0
        np.testing.assert_array_equal(ref.grid, nat.grid)
        np.testing.assert_array_equal(ref.half, np.array(list(nat.bin_sizes.values())) / 2)
    for step in range(8):
        n = int(rng.choice([1, 3, 78, 79, 500, 1025]))
        cmds, bins = ref.sample(n)
        if one_point:
            c2, b2 = _native_sample(ref, key, pos, nat_w, n)
            np.testing.assert_array_equal(b2, bins)
            np.testing.assert_array_equal(c2, cmds)
            np.testing.assert_array_equal(key, ref.mt[0])
            assert int(pos[0]) == ref.mt[1]
        else:
            for c in (nat, py):
                c2, b2 = c.sample(n)
                np.testing.assert_array_equal(b2, bins)
                np.testing.assert_array_equal(c2, cmds)
                c._sync_from_rng()
                np.testing.assert_array_equal(c._mt_key, ref.mt[0])
                assert int(c._mt_pos[0]) == ref.mt[1]
        m = min(n, 200)
        old = rng.integers(0, nb, m)
        old[: m // 3] = old[0]
        old[-1] = nb - 1
        lin, ang = rng.uniform(0, 0.6, m).astype(F32), rng.uniform(0, 0.4, m).astype(F32)
        if m >= 2:
            lin[0], ang[0] = F32(cc.LIN_THR), 0.35
            lin[1], ang[1] = 0.5, np.nextafter(F32(cc.ANG_THR), F32(1))
        r = [0.5, 0.1, 1.0, cc.spacing_range(ref)][step % 4]
        centres = ref.update(old, lin, ang, cc.LIN_THR, cc.ANG_THR, r)
        if one_point:
            _native_update(ref, nat_w, centres, r)
            np.testing.assert_array_equal(nat_w, ref.weights)
        else:
            for c in (nat, py):
                c.update(old, lin, ang, cc.LIN_THR, cc.ANG_THR, local_range=r)
                np.testing.assert_array_equal(c.weights, ref.weights)
                np.testing.assert_array_equal(c.episode_reward_lin, ref.episode_reward_lin)
                np.testing.assert_array_equal(c.episode_reward_ang, ref.episode_reward_ang)


def test_choice_errors_leave_everything():
    """Zero or inf weights: 'contain NaN'; a negative weight: 'not non-negative'.  The generator and every output
    stay; the weights keep the update's adds."""
    n_sums, pair = sim_rows()
    for bad, message in ((None, "probabilities contain NaN"), (-0.5, "probabilities are not non-negative"),
                         (np.inf, "probabilities contain NaN")):
        ref = cc.make_ref("5x2x11", 20, n_sums, seed=3)
        if bad is not None:
            ref.weights[:] = 0.4
            ref.weights[7] = bad
        ref.env_bins[:] = 100
        ref.command_sums[:] = 25.0  # rewards of 1: every entry passes
        ref.commands[:] = 3.0
        before = (ref.mt, ref.commands.copy(), ref.command_sums.copy(), ref.env_bins.copy(), ref.env_bins_f.copy(),
                  ref.command_area.copy())
        info = ref.resample(np.arange(5), 5, 5, 25, pair[0], pair[1], cc.LIN_THR, cc.ANG_THR, 0.1, bad is not None, 1)
        assert info["error"] == message and message in cr.ERROR_CODES
        after = (ref.mt, ref.commands, ref.command_sums, ref.env_bins, ref.env_bins_f, ref.command_area)
        np.testing.assert_array_equal(before[0][0], after[0][0])
        assert before[0][1] == after[0][1]
        for a, b in zip(before[1:], after[1:]):
            np.testing.assert_array_equal(a, b)
        if bad is not None:
            assert ref.weights[100] == 1.0 and ref.weights[7] == bad  # (one add as a centre, five as a neighbour)


@functools.lru_cache(None)
def coverage(gname):
    n_sums, pair = sim_rows()
    cover = cc.Coverage()
    for n, pos, variant in cc.chains_of(gname):
        cc.run_chain(gname, n, pos, variant, n_sums, pair, cover=cover)
    return cover


@pytest.mark.parametrize("gname", list(cc.GRIDS))
def test_chains_reach_every_case(gname):
    c = coverage(gname)
    ref = cc.make_ref(gname, 1, 1)
    assert c.masked > 0 and c.kept > 0, "both arms of the |xy| > 0.2 mask"
    assert c.mask_margin > 1e-6, f"a norm within 1e-6 of 0.2 ({c.mask_margin})"
    assert c.double_add, "a bin with two or more counted adds"
    assert c.clipped, "an add clipped at 1"
    assert all(c.cut), f"a neighbourhood cut by the grid edge on every axis ({c.cut})"
    assert c.all_ones_pass, "a call whose passing bins are all 1.0 already"
    assert c.last_wins_mix, "a bin held by three or more listed envs, passing and failing, all rewards different"
    assert c.corner_bins == set(cc.corners(ref.shape)), "old bins at every corner"
    assert c.placed == {n for n, _, _ in cc.threshold_rewards()}, f"rewards on the thresholds ({c.placed})"
    assert c.weights_seen >= set(cc.ladder().tolist()) - ({0.0} if ref.nb == 1 else set())  # (one bin: never 0 alone)
    assert c.combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {"less", "more", "exact", ("empty", 0, None), ("empty", 1, "prev"), ("empty", 1, "no prev")} <= c.counts
    assert c.lists == {"perm", "full", "upper"}
    assert set(cc.BATCHES) <= c.batch and max(c.batch) == 4096
    assert c.positions == set(cc.POSITIONS)
    assert c.stale > 0 and c.cached > 0
    assert 0 < c.max_passing <= cc.MAX_PASSING


def test_grids_reach_every_leaf_class_and_the_limit():
    """The pairwise sum's leaves over the grids: a plain loop (< 8), 8 lanes with a tail, 8 lanes without, a split;
    the two edge grids sit on the launcher's limit."""
    nbs = {k: cc.make_ref(k, 1, 1).nb for k in cc.GRIDS}
    assert list(nbs.values()) == [1, 6, 110, 128, 129, 5202, cc.MAX_BINS]
    assert cc.make_ref(cc.REFUSED_GRID, 1, 1).nb == cc.MAX_BINS + 1
    assert 16 * cc.MAX_BINS + 2496 <= 124 * 1024 < 16 * (cc.MAX_BINS + 1) + 2496
    leaves = {k: cc.pairwise_tree(nb) for k, nb in nbs.items()}
    assert leaves["2x1x3"] == (1, 1, [6]) and leaves["5x2x11"] == (1, 1, [110]) and leaves["8x2x8"] == (1, 1, [128])
    assert leaves["43x1x3"] == (2, 2, [64, 65])
    assert leaves["51x2x51"][0] == 7 and leaves["10x2x389"][0] == 8
    every = [m for v in leaves.values() for m in v[2]]
    assert any(m < 8 for m in every) and any(m >= 8 and m % 8 for m in every) and any(m >= 8 and m % 8 == 0 for m in every)


def test_serial_walk_is_unreachable_at_the_launchers_limit():
    """Every nb the launcher admits has a tree of at most 8 levels and 64 nodes per level, inside the level tables of
    cd_pairwise_levels (10 levels, 128 nodes): the kernel's serial cd_walk fallback is never taken."""
    shapes = {}
    deepest = widest = 0
    for nb in range(1, cc.MAX_BINS + 1):
        depth, wide, leaves = cc.pairwise_tree(nb)
        assert sum(leaves) == nb and max(leaves) <= 128
        deepest, widest = max(deepest, depth), max(widest, wide)
    assert deepest == 8 and widest == 64
