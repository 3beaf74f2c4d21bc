"""CPU-side checks of the history shift's part of the C ABI (include/lrl_history_shift.h, which include/lrl.h
includes): the two entry points are exported and carry the header's ctypes signature; nothing that existed before
changed, so the ABI version stays.  No device call."""
import ctypes as C
import os
import re

from lrl import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_the_header_is_part_of_lrl_h_and_the_version_stays():
    src = open(os.path.join(INC, "lrl.h")).read()
    assert '#include "lrl_history_shift.h"' in src
    assert re.search(r"#define\s+LRL_ABI_VERSION\s+6\b", src)
    mine = open(os.path.join(INC, "lrl_history_shift.h")).read()
    assert set(_abi.signatures(mine)) == {"lrl_ppo_act_shift", "lrl_sim_history_preshifted"}


def test_entry_points_take_the_headers_signature():
    L = _abi.lib()
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert L.lrl_abi_version() == 6
    assert L.lrl_sim_history_preshifted.argtypes == [vp, i32] and L.lrl_sim_history_preshifted.restype is i32
    # lrl_ppo_act's parameters, then the writable history and the slot width
    assert L.lrl_ppo_act_shift.argtypes == L.lrl_ppo_act.argtypes + [vp, i32]
    assert L.lrl_ppo_act_shift.restype is i32
    assert L.lrl_ppo_act.argtypes == [C.POINTER(_abi.LrlPpoNet), vp, vp, vp, vp, i32, vp, u64, u64, i64, vp, vp, vp, vp,
                                      C.POINTER(_abi.LrlRolloutStore), i32, vp, vp]


def test_null_arguments_are_refused_before_any_launch():
    L = _abi.lib()
    assert L.lrl_sim_history_preshifted(None, 0) == -1  # LRL_E_INVALID
    assert b"null sim" in L.lrl_last_error()
