"""The env step kernel's and observe_kernel's own draws from the counter RNG (observation noise, pushes, the per-step
redraw of motor strength / Kp / Kd) against the Philox restatement of tests/aux_ref.py, on all three builds of the step
kernel (plane, terrain-mesh PGS, terrain-mesh TGS).

Every other env-step test sets STEP_INJECT_UNIFORM and so replaces exactly these draws.  Here each case steps two sims
from the same seed, env offset and state: run A draws in the kernel, run B takes the helpers' uniforms (computed for the
global env id and for the counter after lrl_sim_step's increment) through lrl_sim_inject_uniforms /
lrl_sim_inject_push_uniforms.  Every state and output tensor must be equal bit for bit.  The injected path is pinned to
the reference's recorded outputs elsewhere and carries the arithmetic; what this adds is which uniform reaches which
place.  Kp and Kd have no injection: they, the motor strengths and the pushed velocities are also compared directly with
float32(u * span) + lo.  tests/test_draws_ref.py proves the same two-run design on the CPU oracle.

The parameter blocks (draws_cases.visible_params) give the whole observation row a non-zero noise scale, redraw every
3rd and push every 4th step of an episode; the episode lengths come from a small pool, so in one step some envs are due
and some are not.  Each case prints how many envs were pushed, were redrawn and took a partial last noise block: of 67
envs the first step pushes 29 and redraws 29, the second pushes 10 (14 in a split sim) and redraws 18; every env takes
a partial last block at the widths 42, 45, 49, 51, 229 and 235, none at 48.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import aux_ref as ar
import draws_cases as dc
from helpers import dev, make, make_rough, npy, same, sim_of, stream, sync, vp
from lrl import _abi
from lrl import params as lparams
from obs_layouts import CASES as LAYOUTS
from test_aux_gpu import _randomise_state, set_gentle_terrain

pytestmark = pytest.mark.gpu

F32 = np.float32
i32, i64, u32c = C.c_int32, C.c_int64, C.c_uint32
FLAGS = _abi.STEP_PHYSICS | _abi.STEP_HISTORY
INJECT = _abi.STEP_INJECT_UNIFORM
TENSORS = dict(obs=_abi.T_OBS, hist=_abi.T_OBS_HISTORY, priv=_abi.T_PRIV_OBS, root=_abi.T_ROOT_STATE,
               dof_pos=_abi.T_DOF_POS, dof_vel=_abi.T_DOF_VEL, ms=_abi.T_MOTOR_STRENGTH, kp=_abi.T_KP_FACTOR,
               kd=_abi.T_KD_FACTOR, rew=_abi.T_REWARD, reset=_abi.T_RESET, eplen=_abi.T_EPISODE_LENGTH,
               torques=_abi.T_TORQUES, contact=_abi.T_CONTACT_FORCE, last_root_vel=_abi.T_LAST_ROOT_VEL,
               base_lin_vel=_abi.T_BASE_LIN_VEL, episode_sums=_abi.T_EPISODE_SUMS)

# kind -> (plane or mesh, robot, cfg overrides).  Widths: 42 (NO % 4 = 2), 45 and 49 (1: obs_layouts' lin and yaw_global),
# 48 (0) and 51 (3) from the same switches; 229 (1) and 235 (3) on the mesh builds.
TGS = {"sim.physx.terrain_solver_type": 1}
VEL = {"env.observe_vel": True}
KINDS = {
    "plane42": (False, "mc", {}),
    "plane45": (False, LAYOUTS["lin"][0], LAYOUTS["lin"][2]),
    "plane48": (False, "mc", dict(VEL, **{"env.num_observations": 48})),
    "plane49": (False, LAYOUTS["yaw_global"][0], LAYOUTS["yaw_global"][2]),
    "plane51": (False, "mc", dict(VEL, **{"env.observe_only_lin_vel": True, "env.num_observations": 51})),
    "pgs229": (True, "go1", {}),
    "pgs235": (True, "go1", dict(VEL, **{"env.num_observations": 235})),
    "tgs229": (True, "go1", TGS),
    "tgs235": (True, "go1", dict(VEL, **TGS, **{"env.num_observations": 235})),
}


@functools.lru_cache(None)
def _kind(kind):
    mesh, robot, over = KINDS[kind]
    _, _, M, P = make_rough(robot, **over) if mesh else make(robot, **over)
    assert P.num_obs == int(kind.lstrip("aeglnpst")) and bool(P.terrain_mesh) == mesh
    assert bool(P.terrain_mesh and P.solver_tgs) == kind.startswith("tgs") and P.clip_obs == 100.0
    return mesh, M, P


def _snap(s):
    return {k: npy(s.t(tid)).copy() for k, tid in TENSORS.items()}


def _run(kind, P, n, offset, counter, steps=1, uniforms=None, G=None):
    """``steps`` steps of a fresh sim of ``kind`` with the parameter block ``P`` (and eval block ``G``) from a fixed
    state; ``uniforms``: per step (noise, injected motor-strength column, push uniforms) to inject, None: the kernel
    draws.  Returns per step the snapshots before and after it."""
    mesh, M, _ = _kind(kind)
    rng = np.random.default_rng(17)
    out = []
    with sim_of(M, P, n, offset, dc.SEED) as s:
        if mesh:
            set_gentle_terrain(s)
        if G is not None:
            _abi.check(s.L.lrl_sim_set_eval_group(s.h, C.byref(G)))
        _randomise_state(s, rng, (2.0, 6.0))
        # Kp / Kd factors outside every redraw range: an env that keeps them shows it
        s.t(_abi.T_KP_FACTOR).copy_(dev(np.repeat(rng.uniform(1.35, 1.45, (n, 1)), 12, 1)))
        s.t(_abi.T_KD_FACTOR).copy_(dev(np.repeat(rng.uniform(1.55, 1.65, (n, 1)), 12, 1)))
        s.t(_abi.T_EPISODE_LENGTH).copy_(dev(dc.EPLEN_POOL[np.arange(n) % len(dc.EPLEN_POOL)], torch.int32))
        actions = [dev(rng.uniform(-1.5, 1.5, (n, 12))) for _ in range(steps)]
        _abi.check(s.L.lrl_sim_set_step_counter(s.h, i64(counter)))
        for k in range(steps):
            before = _snap(s)
            flags = FLAGS
            if uniforms is not None:
                keep = [dev(u) for u in uniforms[k]]
                _abi.check(s.L.lrl_sim_inject_uniforms(s.h, vp(keep[0]), vp(keep[1])))
                _abi.check(s.L.lrl_sim_inject_push_uniforms(s.h, vp(keep[2])))
                flags |= INJECT
            _abi.check(s.L.lrl_sim_step(s.h, vp(actions[k]), u32c(flags), stream()))
            sync()
            out.append((before, _snap(s)))
    return out


def _check_case(kind, P, n, offset, counter, steps=1, G=None, n_train=None, with_zero_noise=False):
    """Run A against run B and against the helpers' values; returns per step (redraw, push) masks."""
    NO = P.num_obs
    blocks = dc.blocks_of(P, G, n, n if n_train is None else n_train)
    ref = [dc.step_uniforms(blocks, NO, offset, counter + k + 1, dc.SEED) for k in range(steps)]
    A = _run(kind, P, n, offset, counter, steps, None, G)
    B = _run(kind, P, n, offset, counter, steps, [(nz, dc.injected_ms(du), pu) for nz, du, _, pu in ref], G)
    masks = []
    for k, ((before, a), (before_b, b), (noise, dr_u, word, push_u)) in enumerate(zip(A, B, ref)):
        what = f"{kind} n={n} offset={offset} counter={counter + k + 1:#x}"
        for t in TENSORS:
            same(before_b[t], before[t], f"{what}: start of the step, {t}")
            assert np.isfinite(a[t]).all() if a[t].dtype == F32 else True, (what, t)
        for t in TENSORS:
            same(a[t], b[t], f"{what}: drawn vs injected, {t}")
        H = a["hist"].shape[1]
        same(a["hist"][:, H - NO:], a["obs"], f"{what}: newest history slot")
        assert np.abs(b["obs"]).max() < P.clip_obs, f"{what}: an obs entry sits at the clip"
        redraw, push = dc.due(blocks, P.rand_interval, before["eplen"])
        same(a["eplen"], before["eplen"] + 1, f"{what}: episode length")
        # the redraw, directly: each env its own group's switch, word, span and low end
        for col, t, rng_name in ((0, "ms", "motor_strength_range"), (1, "kp", "kp_range"), (2, "kd", "kd_range")):
            want = before[t].copy()
            for e in np.flatnonzero(redraw):
                Bk = blocks[e]
                if word[e, col] >= 0:
                    want[e, :] = ar.draw32(dr_u[e, col], Bk.dr_span[col], getattr(Bk, rng_name)[0])
            same(a[t], want, f"{what}: {t} (redrawn rows the helper's word, the others kept)")
        # the push, directly: root velocity x, y = float32(span * u) + lo of the env's group
        for e in np.flatnonzero(push):
            same(a["root"][e, 7:9], ar.draw32(push_u[e], blocks[e].push_span, blocks[e].push_lo), f"{what}: push {e}")
        masks.append((redraw, push))
        tail = n if NO % 4 else 0
        print(f"{what}: {int(push.sum())} of {n} envs pushed, {int(redraw.sum())} redrawn, {tail} took a partial "
              f"last noise block ({NO % 4} of 4 words)")
    if steps > 1:  # the next counter: other draws (in the reference, so by the equalities above in the kernel)
        assert (ref[0][0] != ref[1][0]).mean() > 0.95 and (ref[0][3] != ref[1][3]).all()
        assert (A[0][1]["obs"] != A[1][1]["obs"]).mean() > 0.95
    if with_zero_noise:
        Z = _run(kind, dc.visible_params(P, zero_noise=True), n, offset, counter, 1, None, G)
        differ = (Z[0][1]["obs"] != A[0][1]["obs"]).mean()
        assert differ > 0.95, f"{kind}: the noise shows in only {differ:.3f} of the obs entries"
        same(Z[0][1]["root"], A[0][1]["root"], f"{kind}: the noise scale reaches the obs rows alone")
    return masks


def _assert_mixed(masks, n):
    redraw, push = masks[0]
    assert redraw.sum() >= n / 4 and push.sum() >= n / 4, (redraw.sum(), push.sum())
    assert (~redraw).sum() >= n / 4 and (~push).sum() >= n / 4  # and envs not due, which keep their values


@pytest.mark.parametrize("kind", ["plane42", "pgs229", "tgs229"])
def test_each_build_draws_what_the_helpers_inject(kind):
    """67 envs (padded env slots in the last workgroup), env offset 0, counter 0; and the noise scale zeroed changes
    more than 95 % of the obs entries, so the comparison sees the noise."""
    P = dc.visible_params(_kind(kind)[2])
    _assert_mixed(_check_case(kind, P, 67, 0, 0, with_zero_noise=True), 67)


@pytest.mark.parametrize("kind", ["plane45", "plane48", "plane49", "plane51", "pgs235", "tgs235"])
def test_row_widths_and_the_wrapping_counter(kind):
    """Every NO % 4, env offset 1000, and the counter (5 << 32) + 0xFFFFFFFF: the step's increment wraps the low word
    and carries into the word XORed into the key; then a second step on the next counter."""
    P = dc.visible_params(_kind(kind)[2])
    _assert_mixed(_check_case(kind, P, 67, 1000, dc.WRAP, steps=2), 67)


@pytest.mark.parametrize("kind", ["plane42", "pgs229", "tgs229"])
def test_one_env_at_an_offset_past_2_31(kind):
    """n = 1 (every other env slot of the workgroup is padding); lrl_sim_create accepts an env offset >= 2^31, whose
    low 32 bits are the key."""
    P = dc.visible_params(_kind(kind)[2])
    assert dc.BIG_OFFSET >= 2 ** 31
    (redraw, push), _ = _check_case(kind, P, 1, dc.BIG_OFFSET, dc.WRAP, steps=2)
    assert redraw.all() and push.all()


@pytest.mark.parametrize("ms,kp,kd", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
def test_redraw_switches_hand_out_the_words_in_order(ms, kp, kd):
    """All eight switch combinations on the plane build: a switch that is off consumes no word (with ms off Kp takes
    word 0; with ms on, injected or not, Kp takes word 1)."""
    P = dc.visible_params(_kind("plane42")[2], ms, kp, kd)
    u, word = ar.dr_uniforms(1000, 1, dc.SEED, ms, kp, kd)
    if kp:
        assert word[1] == (1 if ms else 0)
    if kd:
        assert word[2] == ms + kp
    _assert_mixed(_check_case("plane42", P, 67, 1000, 0), 67)


@pytest.mark.parametrize("kind", ["plane42", "pgs229", "tgs229"])
def test_split_sim_draws_per_group(kind):
    """One sim with an eval group from env 29 on (inside a wave on every build): train (ms, kd), eval (kp, kd), disjoint
    ranges, push intervals 4 and 3 with different spans.  Each env takes its own group's word index, span and low
    end."""
    n, n_train = 67, 29
    P = dc.visible_params(_kind(kind)[2], True, False, True)
    P.num_train_envs = n_train
    # the eval block as LeggedRobotEnv(cfg, eval_cfg) forms it (test_eval_group_gpu._split): from the two groups' blocks
    G = lparams.eval_group_params(P, dc.eval_block(dc.copy_params(P)))
    assert G is not None and (G.randomize_motor_strength, G.randomize_kp, P.randomize_kp, G.push_interval, P.push_interval) == \
        (0, 1, 0, 3, 4)
    u_tr, w_tr = ar.dr_uniforms(0, 1, dc.SEED, 1, 0, 1)
    u_ev, w_ev = ar.dr_uniforms(n_train, 1, dc.SEED, 0, 1, 1)
    assert w_tr.tolist() == [0, -1, 1] and w_ev.tolist() == [-1, 0, 1]
    masks = _check_case(kind, P, n, 1000, dc.WRAP, steps=2, G=G, n_train=n_train)
    for rows in (np.arange(n) < n_train, np.arange(n) >= n_train):
        redraw, push = masks[0]
        assert redraw[rows].sum() >= 4 and push[rows].sum() >= 4 and (~push[rows]).sum() >= 4
    # the groups push on different steps of the same episode lengths
    tr, ev = np.arange(n) < n_train, np.arange(n) >= n_train
    L = dc.EPLEN_POOL[np.arange(n) % len(dc.EPLEN_POOL)] + 1
    assert np.array_equal(masks[0][1][tr], L[tr] % 4 == 0) and np.array_equal(masks[0][1][ev], L[ev] % 3 == 0)


# =================================================================================================================
# observe_kernel
# =================================================================================================================
WRITTEN = ("obs", "priv", "base_lin_vel", "last_root_vel")


@pytest.mark.parametrize("kind", ["plane42", "plane51", "pgs229", "pgs235"])
def test_observe_kernel_draws_what_the_helpers_inject(kind):
    """lrl_sim_observe_idx on 9 permuted ids and the _dev form with a count below its bound, at a counter set after a
    step (observe does not increment it): the rows drawn by observe_kernel equal the rows with obs_noise_uniforms of
    that counter injected, bit for bit; rows not listed stay untouched."""
    mesh, M, P0 = _kind(kind)
    P = dc.visible_params(P0)
    n, offset, NO = 67, 1000, P.num_obs
    counter = (9 << 32) + 77
    rng = np.random.default_rng(23)
    noise = np.stack([ar.obs_noise_uniforms(offset + e, counter, dc.SEED, NO) for e in range(n)])
    with sim_of(M, P, n, offset, dc.SEED) as s:
        if mesh:
            set_gentle_terrain(s)
        _randomise_state(s, rng, (2.0, 6.0))
        actions = dev(rng.uniform(-1.5, 1.5, (n, 12)))
        _abi.check(s.L.lrl_sim_step(s.h, vp(actions), u32c(FLAGS), stream()))
        sync()
        stepped = npy(s.t(_abi.T_OBS)).copy()
        _abi.check(s.L.lrl_sim_set_step_counter(s.h, i64(counter)))
        H = s.t(_abi.T_OBS_HISTORY).shape[1]
        dnoise, ddr = dev(noise), dev(np.full(n, 0.5, F32))
        _abi.check(s.L.lrl_sim_inject_uniforms(s.h, vp(dnoise), vp(ddr)))
        some = rng.permutation(n)[:9].astype(np.int32)
        dsome, dcount = dev(some, torch.int32), dev([5], torch.int32)

        def observe(flags, counted):
            for t in WRITTEN:
                s.t(TENSORS[t]).fill_(-99.0)
            s.t(_abi.T_OBS_HISTORY)[:, H - NO:] = -99.0
            if counted:
                _abi.check(s.L.lrl_sim_observe_idx_dev(s.h, vp(dsome), i32(9), vp(dcount), u32c(flags), stream()))
            else:
                _abi.check(s.L.lrl_sim_observe_idx(s.h, vp(dsome), i32(9), u32c(flags), stream()))
            sync()
            return _snap(s)

        for counted, ids in ((False, some), (True, some[:5])):
            drawn, injected = observe(FLAGS, counted), observe(FLAGS | INJECT, counted)
            what = f"{kind} observe{'_dev' if counted else ''}"
            rest = np.setdiff1d(np.arange(n), ids)
            for t in TENSORS:
                same(drawn[t], injected[t], f"{what}: drawn vs injected, {t}")
            for t in WRITTEN:
                assert (drawn[t][rest] == -99.0).all(), f"{what}: {t} rows of envs not listed"
                assert (drawn[t][ids] != -99.0).all() and np.isfinite(drawn[t][ids]).all()
            assert (drawn["hist"][rest, H - NO:] == -99.0).all()
            same(drawn["hist"][ids, H - NO:], drawn["obs"][ids], f"{what}: newest history slot")
            assert np.abs(drawn["obs"][ids]).max() < P.clip_obs
            # the same state at another counter: other noise than the step's own rows
            assert (drawn["obs"][ids] != stepped[ids]).mean() > 0.95
        print(f"{kind} observe: 9 and 5 rows, each with a partial last noise block of {NO % 4} words")
