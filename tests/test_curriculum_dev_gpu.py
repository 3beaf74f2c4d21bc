"""curriculum_dev_kernel (csrc/lrl_curriculum_dev.hip) through lrl_sim_curriculum_resample_dev against numpy itself
(tests/curriculum_ref.py: a real RandomState, np.sum, RandomState.choice / uniform, the update as the cited code writes
it), on sims made with lrl_sim_create and caller-owned buffers in an lrl_dev_curriculum.

Every buffer the contract names is compared bit for bit after every call of every chain: weights, the cdf cache,
state[0..3], the MT19937 key and position, episode_reward_lin / _ang, env_bins, env_bins_f, command_area, the command
rows and command_sums; commands' column 3 and every env outside ids[:n] are compared with their pre-call values.  The
chains (tests/curriculum_cases.py) cover batches of 1 .. 4096 envs, generator positions 624, 0, 620 and 623, id lists
and device counts of every kind, and the update inputs listed there; tests/test_curriculum_ref.py asserts on the CPU
that they reach each case.  The one comparison that is not exact by construction is the |xy| > 0.2 mask (float32 on
the device, a float64 norm of the float32 commands in the reference); its condition, asserted here and on the CPU:
no drawn norm lies within 1e-6 of 0.2.  No test passes an env id outside [0, n) or a scratch buffer smaller than
lrl.h asks for.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import curriculum_cases as cc
import curriculum_ref as cr
from helpers import DEV, _mc, dev, mc_sim, npy, stream, sync, vp
from lrl import _abi

pytestmark = pytest.mark.gpu

F32 = np.float32
i32 = C.c_int32
PAIR = (0, 1)  # the Mini Cheetah preset's (tracking_lin_vel, tracking_ang_vel) sum rows (lrl/env.py's _track_rows)
SPARE = 77     # state[3]: never written


def exact(got, want, what):
    """Bit-for-bit equality of two arrays (signed zeros and NaN payloads included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


class Bench:
    """A sim, an lrl_dev_curriculum of torch buffers mirroring a CurriculumRef, and the comparison of the two."""

    def __init__(self, s, ref):
        self.s, self.N, self.nb = s, s.n, ref.nb
        assert len(ref.env_bins) == s.n and ref.command_sums.shape[0] == s.t(_abi.T_COMMAND_SUMS).shape[0]
        assert tuple(s.t(_abi.T_COMMANDS).shape) == (s.n, 4)
        N, nb = self.N, self.nb
        f64, i64 = torch.float64, torch.int64
        key, pos = ref.mt
        self.b = dict(
            weights=dev(ref.weights, f64), cdf=torch.full((nb,), -3.0, dtype=f64, device=DEV),
            state=dev([0, pos, 0, SPARE], torch.int32), mt_key=dev(key.view(np.int32), torch.int32),
            ep_rew_lin=dev(ref.episode_reward_lin, f64), ep_rew_ang=dev(ref.episode_reward_ang, f64),
            env_bins=torch.zeros(N, dtype=i64, device=DEV), env_bins_f=torch.zeros(N, device=DEV),
            command_area=torch.zeros(1, dtype=f64, device=DEV), axes=dev(np.concatenate(ref.axes), f64),
            words=torch.zeros(8 * N, dtype=torch.int32, device=DEV), draws=torch.zeros(4 * N, dtype=f64, device=DEV),
            prev_bins_f=torch.zeros(N, device=DEV), prev_area=torch.zeros(1, dtype=f64, device=DEV))
        d = _abi.LrlDevCurriculum()
        for k in ("weights", "cdf", "state", "mt_key", "ep_rew_lin", "ep_rew_ang", "env_bins", "env_bins_f",
                  "command_area", "axes", "words", "draws"):
            setattr(d, k, self.b[k].data_ptr())
        d.half[:] = [float(h) for h in ref.half]
        d.nx, d.ny, d.nz = ref.shape
        self.desc = d
        self.cdf = np.full(nb, -3.0)  # what the device cdf buffer must hold
        self.state0 = 0

    def fill(self, ref, call):
        """The call's pre-call values (the reference holds them already) and sentinels into the device buffers."""
        s, b = self.s, self.b
        s.t(_abi.T_COMMANDS).copy_(dev(ref.commands))
        s.t(_abi.T_COMMAND_SUMS).copy_(dev(ref.command_sums))
        b["env_bins"].copy_(dev(ref.env_bins, torch.int64))
        b["env_bins_f"].copy_(dev(ref.env_bins_f))
        b["command_area"].copy_(dev(ref.command_area, torch.float64))
        b["words"].fill_(-1)
        b["draws"].fill_(-5.0)
        if call.get("special") == "stale cdf":
            b["cdf"].fill_(-3.0)
            b["state"][0] = 0
            self.cdf, self.state0 = np.full(self.nb, -3.0), 0
        prev = call.get("special") == "prev"
        if prev:
            b["prev_bins_f"].copy_(dev(call["prev_bins_f"]))
            b["prev_area"].copy_(dev([call["prev_area"]], torch.float64))
        self.desc.env_bins_f_prev = b["prev_bins_f"].data_ptr() if prev else None
        self.desc.command_area_prev = b["prev_area"].data_ptr() if prev else None
        self.pre = dict(commands=ref.commands.copy(), sums=ref.command_sums.copy(), env_bins=ref.env_bins.copy())

    def launch(self, call):
        ids, count = dev(call["ids"], torch.int32), dev([call["count"]], torch.int32)
        assert len(call["ids"]) >= call["nmax"] and call["nmax"] <= self.N
        assert call["ids"].min() >= 0 and call["ids"].max() < self.N
        rc = self.s.L.lrl_sim_curriculum_resample_dev(
            self.s.h, C.byref(self.desc), vp(ids), i32(call["nmax"]), vp(count), i32(call["ep_len"]),
            i32(call["rows"][0]), i32(call["rows"][1]), C.c_double(cc.LIN_THR), C.c_double(cc.ANG_THR),
            C.c_double(call["local_range"]), i32(call["update"]), i32(call["log_area"]), stream())
        sync()
        return rc

    def device(self):
        b, s = self.b, self.s
        out = {k: npy(b[k]) for k in ("weights", "cdf", "state", "ep_rew_lin", "ep_rew_ang", "env_bins", "env_bins_f",
                                      "command_area")}
        out["mt_key"] = npy(b["mt_key"]).view(np.uint32)
        out["commands"] = npy(s.t(_abi.T_COMMANDS))
        out["sums"] = npy(s.t(_abi.T_COMMAND_SUMS))
        return out

    def compare(self, ref, call, info, what):
        """The device buffers after the call against the reference after it."""
        if info["n"] and info["error"] is None:
            margin = np.abs(info["norm"] - 0.2).min()
            assert margin > 1e-6, f"{what}: a drawn norm within 1e-6 of 0.2 ({margin})"
            if call.get("special") == "stale cdf" or (info["centres"] is not None and len(info["centres"])):
                self.cdf = ref.cdf  # recomputed: numpy's p.cumsum() / cumsum[-1]
            self.state0 = 1
        elif info["n"]:
            self.state0 = 0
        got = self.device()
        key, pos = ref.mt
        code = cr.ERROR_CODES[info["error"]] if info["error"] else 0
        exact(got["mt_key"], key, f"{what}: MT19937 key")
        exact(got["state"], np.array([self.state0, pos, code, SPARE], np.int32), f"{what}: state (cdf valid, MT position, "
              "error, spare)")
        exact(got["weights"], ref.weights, f"{what}: weights")
        exact(got["cdf"], self.cdf, f"{what}: cdf cache")
        exact(got["ep_rew_lin"], ref.episode_reward_lin, f"{what}: episode_reward_lin")
        exact(got["ep_rew_ang"], ref.episode_reward_ang, f"{what}: episode_reward_ang")
        exact(got["env_bins"], ref.env_bins, f"{what}: env_bins")
        exact(got["env_bins_f"], ref.env_bins_f, f"{what}: env_bins_f")
        exact(got["command_area"], ref.command_area, f"{what}: command_area")
        exact(got["commands"], ref.commands, f"{what}: commands")
        exact(got["sums"], ref.command_sums, f"{what}: command_sums")
        # what no call may touch, against the pre-call values
        rest = np.setdiff1d(np.arange(self.N), call["ids"][:info["n"]])
        exact(got["commands"][:, 3], self.pre["commands"][:, 3], f"{what}: commands column 3")
        exact(got["commands"][rest], self.pre["commands"][rest], f"{what}: commands of envs not listed")
        exact(got["sums"][:, rest], self.pre["sums"][:, rest], f"{what}: command_sums of envs not listed")
        exact(got["env_bins"][rest], self.pre["env_bins"][rest], f"{what}: env_bins of envs not listed")
        return got


@pytest.mark.parametrize("gname", list(cc.GRIDS))
def test_chains_match_numpy(gname):
    """Every chain of the grid: eleven calls on one sim, the device's MT19937 stream continuing from call to call."""
    n_sums = _mc()[3].num_sum_keys + 5  # (Bench checks it against the sim's table)
    with contextlib.ExitStack() as stack:
        for n, pos, variant in cc.chains_of(gname):
            bench = {}

            def hook(ref, call, phase, info):
                if phase == "init":
                    ref.episode_reward_lin[:] = 7.0
                    ref.episode_reward_ang[:] = -7.0
                    bench["s"] = stack.enter_context(mc_sim(call["N"]))
                    bench["b"] = Bench(bench["s"], ref)
                elif phase == "before":
                    bench["b"].fill(ref, call)
                else:
                    what = f"{gname} n={n} pos={pos} variant={variant} call {call['k']}"
                    assert bench["b"].launch(call) == 0, what
                    bench["b"].compare(ref, call, info, what)

            cc.run_chain(gname, n, pos, variant, n_sums, PAIR, hook=hook)
            stack.close()


def _call(ids, ep_len=25, update=1, log_area=1, local_range=0.1, count=None, rows=PAIR):
    ids = np.asarray(ids, np.int32)
    return dict(ids=ids, count=len(ids) if count is None else count, nmax=len(ids), ep_len=ep_len, rows=rows,
                update=update, log_area=log_area, local_range=local_range, special=None)


def _fresh(rng, ref, passing_ids=(), ep_len=25):
    """Known pre-call values in the reference: random commands / sums / log buffers, failing rewards except for
    passing_ids."""
    N, nb = len(ref.env_bins), ref.nb
    ref.commands[:] = rng.uniform(-9, 9, (N, 4)).astype(F32)
    ref.command_sums[:] = rng.uniform(-50, 50, ref.command_sums.shape).astype(F32)
    ref.command_sums[PAIR[0]] = rng.uniform(0, 0.2 * ep_len, N).astype(F32)
    ref.command_sums[PAIR[1]] = rng.uniform(0, 0.1 * ep_len, N).astype(F32)
    for e in passing_ids:
        ref.command_sums[PAIR[0], e], ref.command_sums[PAIR[1], e] = 0.5 * ep_len, 0.4 * ep_len
    ref.env_bins_f[:] = rng.uniform(-9, 9, N).astype(F32)
    ref.command_area[0] = rng.uniform(2, 3)


@pytest.mark.parametrize("gname", ["5x2x11", "43x1x3", "51x2x51"])
@pytest.mark.parametrize("bad", ["zero", "negative", "inf"])
def test_error_states(gname, bad):
    """Weights RandomState.choice refuses: state[2] names numpy's message, state[0] = 0, the generator, commands,
    command_sums, env bins and log buffers stay, the weights keep the update's adds; after a repair the next call
    succeeds and matches."""
    N = 67
    rng = np.random.default_rng([list(cc.GRIDS).index(gname), len(bad)])
    with mc_sim(N) as s:
        ref = cc.make_ref(gname, N, s.t(_abi.T_COMMAND_SUMS).shape[0], pos=620, seed=5)
        nb = ref.nb
        bad_bin = nb // 2
        if bad == "zero":
            passing = []
        else:
            ref.weights[:] = cc.ladder()[rng.integers(1, 6, nb)]
            ref.weights[bad_bin] = -0.5 if bad == "negative" else np.inf
            passing = [3, 11, 40]
        ref.episode_reward_lin[:], ref.episode_reward_ang[:] = 7.0, -7.0
        b = Bench(s, ref)
        ids = rng.permutation(N)[:20]
        passing = [int(e) for e in ids[:len(passing)]]
        ref.env_bins[:] = rng.integers(0, nb, N)
        ref.env_bins[ref.env_bins == bad_bin] = 0  # (local_range 0.1 reaches the centre only: the bad weight stays)
        _fresh(rng, ref, passing)
        w0 = ref.weights.copy()
        call = _call(ids)
        before = (ref.mt, ref.commands.copy(), ref.command_sums.copy(), ref.env_bins.copy(), ref.env_bins_f.copy(),
                  ref.command_area.copy())
        b.fill(ref, call)
        info = cc.apply(ref, call)
        assert info["error"] == ("probabilities are not non-negative" if bad == "negative"
                                 else "probabilities contain NaN")
        assert len(info["centres"]) == len(passing) and (bad == "zero" or (ref.weights != w0).any())
        assert b.launch(call) == 0
        got = b.compare(ref, call, info, f"{gname} {bad}: refused")
        assert got["state"][0] == 0 and got["state"][2] == (2 if bad == "negative" else 1)
        exact(got["mt_key"], before[0][0], "the key stays")
        assert got["state"][1] == before[0][1] == 620
        for k, v in zip(("commands", "sums", "env_bins", "env_bins_f", "command_area"), before[1:]):
            exact(got[k], v, f"{gname} {bad}: {k} stays")
        # the repair: a valid weight (the host clears the error code), then a call that succeeds
        if bad == "zero":
            ref.weights[[1 % nb, nb - 1]] = [0.2, 0.6000000000000001]
        else:
            ref.weights[bad_bin] = 0.4
        b.b["weights"].copy_(dev(ref.weights, torch.float64))
        b.b["state"][2] = 0
        _fresh(rng, ref, passing)
        call = _call(ids, update=int(bad != "zero"), local_range=0.5)
        b.fill(ref, call)
        info = cc.apply(ref, call)
        assert info["error"] is None
        assert b.launch(call) == 0
        b.cdf = ref.cdf  # state[0] was 0: recomputed
        got = b.compare(ref, call, info, f"{gname} {bad}: repaired")
        assert got["state"].tolist() == [1, ref.mt[1], 0, SPARE] and ref.mt[1] != 620


def test_refusals_launch_nothing():
    """One bin past the launcher's limit (31 x 1 x 251 = 7781), and bad arguments: a non-zero return code and every
    buffer as it was."""
    N = 67
    rng = np.random.default_rng(3)
    with mc_sim(N) as s:
        n_sums = s.t(_abi.T_COMMAND_SUMS).shape[0]
        for grid in (cc.REFUSED_GRID, cc.GRIDS["5x2x11"]):
            ref = cc.make_ref(grid, N, n_sums, seed=9)
            ref.weights[:] = cc.ladder()[rng.integers(1, 6, ref.nb)]
            ref.env_bins[:] = rng.integers(0, ref.nb, N)
            _fresh(rng, ref, [1, 2, 3])
            b = Bench(s, ref)
            good = _call(rng.permutation(N)[:20])
            b.fill(ref, good)
            before = b.device()
            if grid is cc.REFUSED_GRID:
                assert ref.nb == cc.MAX_BINS + 1
                attempts = [good]
            else:
                attempts = [dict(good, rows=(n_sums, 0)), dict(good, rows=(0, -1)), dict(good, ep_len=0),
                            dict(good, nmax=-1)]
            for call in attempts:
                assert b.launch(call) != 0, call
                after = b.device()
                for k in before:
                    exact(after[k], before[k], f"refused: {k}")
            for k in ("weights", "cdf", "state", "mt_key", "ep_rew_lin", "axes", "words", "draws"):
                d = _abi.LrlDevCurriculum.from_buffer_copy(b.desc)
                setattr(d, k, None)
                ids, count = dev(good["ids"], torch.int32), dev([20], torch.int32)
                assert s.L.lrl_sim_curriculum_resample_dev(
                    s.h, C.byref(d), vp(ids), i32(20), vp(count), i32(25), i32(0), i32(1), C.c_double(0.3),
                    C.c_double(0.2), C.c_double(0.5), i32(1), i32(1), stream()) != 0, k
            sync()
            after = b.device()
            for k in before:
                exact(after[k], before[k], f"null {k}: refused")


def _untemper(y):
    """The key word MT19937's output tempering maps to y (numpy confirms the draws below)."""
    y ^= y >> 18
    y ^= (y << 15) & 0xefc60000
    x = y
    for _ in range(5):
        x = y ^ ((x << 7) & 0x9d2c5680)
    y = x & 0xffffffff
    x = y
    for _ in range(3):
        x = y ^ (x >> 11)
    return x & 0xffffffff


def test_draws_equal_to_a_cdf_value_go_right():
    """searchsorted(side='right'): a draw that equals a cdf value exactly takes the first bin whose cdf exceeds it.
    Random draws never land there, so the key is made to: weights 1 1 0 0 1 1 give the cdf 0.25 0.5 0.5 0.5 0.75 1,
    and the first three doubles of the stream are 0.5, 0.25 and 0.75."""
    N = 8
    rng = np.random.default_rng(21)
    with mc_sim(N) as s:
        ref = cc.make_ref("2x1x3", N, s.t(_abi.T_COMMAND_SUMS).shape[0], pos=0, seed=4)
        key = ref.mt[0].copy()
        for j, word in enumerate((0x80000000, 0x40000000, 0xC0000000)):
            key[2 * j], key[2 * j + 1] = _untemper(word), 0
        ref.rng.set_state(("MT19937", key, 0))
        probe = np.random.RandomState()
        probe.set_state(ref.rng.get_state())
        assert probe.random_sample(3).tolist() == [0.5, 0.25, 0.75]
        ref.weights[:] = [1, 1, 0, 0, 1, 1]
        ref.env_bins[:] = 2
        _fresh(rng, ref)
        b = Bench(s, ref)
        call = _call(rng.permutation(N), update=0, log_area=0)
        b.fill(ref, call)
        info = cc.apply(ref, call)
        assert ref.cdf.tolist() == [0.25, 0.5, 0.5, 0.5, 0.75, 1.0]
        assert ref.env_bins[call["ids"][:3]].tolist() == [4, 1, 5]
        assert b.launch(call) == 0
        b.cdf = ref.cdf  # state[0] was 0
        b.compare(ref, call, info, "draws on cdf values")
