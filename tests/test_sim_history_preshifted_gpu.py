"""lrl_sim_history_preshifted: the next lrl_sim_step with LRL_STEP_HISTORY leaves rows [0, rows) of the history buffer
to the caller, who shifted them already (lrl_ppo_act_shift does, while copying them into the rollout storage), and
shifts rows [rows, n) itself; the count holds for one step.

Two sims made alike: one takes a plain LRL_STEP_HISTORY step; on the other the first `rows` history rows are shifted
with torch, the call is made, then the same step.  Every tensor of the sim must then be the same bits.  A second step
without the call shifts every row again (one-shot).  5 envs is not a multiple of the env kernel's 4 envs per wave.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DEV, dev, mc_sim, npy, same, stream, sync, vp
from lrl import _abi

pytestmark = pytest.mark.gpu

F32 = np.float32
FLAGS = C.c_uint32(_abi.STEP_HISTORY)


def _fill(s):
    """History rows with a value unique to (env, column), exact in float32."""
    n, H = s.n, s.P.num_obs * s.P.num_history
    old = (np.arange(n)[:, None] * 1024 + np.arange(H)[None]).astype(F32)
    s.t(_abi.T_OBS_HISTORY).copy_(dev(old))
    return old


def _state(s):
    """Every tensor the sim exposes (the ones without storage in this configuration left out), as numpy copies."""
    sync()
    out = {}
    for tid in range(_abi.T_NUM):
        d = _abi.LrlTensor()
        _abi.check(s.L.lrl_sim_tensor(s.h, C.c_int32(tid), C.byref(d)))
        if d.data and all(d.shape[i] > 0 for i in range(d.ndim)):
            out[tid] = npy(s.t(tid)).copy()
    assert _abi.T_OBS_HISTORY in out and _abi.T_OBS in out and _abi.T_ROOT_STATE in out
    return out


def _step(s, actions):
    _abi.check(s.L.lrl_sim_step(s.h, vp(actions), FLAGS, stream()))


@pytest.mark.parametrize("n", [8, 5])
@pytest.mark.parametrize("rows", ["0", "3", "all"])
def test_preshifted_rows_are_left_alone_and_the_rest_shifted(n, rows):
    rows = {"0": 0, "3": 3, "all": n}[rows]
    actions = torch.zeros(n, 12, device=DEV)
    with mc_sim(n) as a, mc_sim(n) as b:
        NO, H = a.P.num_obs, a.P.num_obs * a.P.num_history
        old = _fill(a)
        _fill(b)
        _step(a, actions)
        hb = b.t(_abi.T_OBS_HISTORY)
        hb[:rows, : H - NO] = hb[:rows, NO:].clone()
        _abi.check(b.L.lrl_sim_history_preshifted(b.h, C.c_int32(rows)))
        _step(b, actions)
        sa, sb = _state(a), _state(b)
        same(sa[_abi.T_OBS_HISTORY][:, : H - NO], old[:, NO:], "plain step: shifted part")
        same(sa[_abi.T_OBS_HISTORY][:, H - NO:], sa[_abi.T_OBS], "plain step: newest slot")
        for tid in sa:
            same(sb[tid], sa[tid], f"tensor {tid} after the preshifted step (rows {rows} of {n})")
        # one-shot: the next step shifts every row again, as the plain sim's does
        before = sa[_abi.T_OBS_HISTORY]
        _step(a, actions)
        _step(b, actions)
        sa, sb = _state(a), _state(b)
        same(sb[_abi.T_OBS_HISTORY][:, : H - NO], before[:, NO:], "second step: every row shifted")
        for tid in sa:
            same(sb[tid], sa[tid], f"tensor {tid} after the second step")


def test_a_step_without_the_history_flag_keeps_the_count():
    """The count is consumed by the next step that shifts: a step without LRL_STEP_HISTORY launches no shift and leaves
    it standing."""
    n = 5
    actions = torch.zeros(n, 12, device=DEV)
    with mc_sim(n) as s:
        NO, H = s.P.num_obs, s.P.num_obs * s.P.num_history
        old = _fill(s)
        _abi.check(s.L.lrl_sim_history_preshifted(s.h, C.c_int32(n)))
        _abi.check(s.L.lrl_sim_step(s.h, vp(actions), C.c_uint32(0), stream()))
        sync()
        same(npy(s.t(_abi.T_OBS_HISTORY)), old, "no history flag: history untouched")
        _step(s, actions)
        sync()
        same(npy(s.t(_abi.T_OBS_HISTORY))[:, : H - NO], old[:, : H - NO], "all rows preshifted: nothing shifted")


def test_out_of_range_counts_are_refused():
    with mc_sim(5) as s:
        for rows in (-1, 6, 2 ** 31 - 1):
            assert s.L.lrl_sim_history_preshifted(s.h, C.c_int32(rows)) == -1  # LRL_E_INVALID
            assert b"lrl_sim_history_preshifted" in s.L.lrl_last_error()
        assert s.L.lrl_sim_history_preshifted(None, C.c_int32(0)) == -1
        _abi.check(s.L.lrl_sim_history_preshifted(s.h, C.c_int32(5)))
        _abi.check(s.L.lrl_sim_history_preshifted(s.h, C.c_int32(0)))
