"""CPU-side checks of the navigation wrapper's native step (include/lrl.h lrl_nav_*, lrl/high_level.py native=True):
the symbols and the ABI version, the ctypes mirror of lrl_nav_state against the constants lrl.h documents beside the
struct and against the C compiler's layout, and the refusal of a low-level env without a sim.  The step itself is
checked on the GPU (tests/test_nav_native_gpu.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, golden
from lrl import _abi

sys.path.insert(0, GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lrl.h")


def _defines():
    src = open(HDR).read()
    return {k: int(v, 0) for k, v in re.findall(r"#define (LRL_NAV_[A-Z_]+) (0x[0-9a-fA-F]+|\d+)u?\b", src)}


def test_nav_symbols_and_abi_version():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("liblrl.so not built")
    L = _abi.lib()
    assert L.lrl_abi_version() == 6
    for name in ("lrl_nav_begin_step", "lrl_nav_end_step"):
        assert getattr(L, name).restype is C.c_int32


def test_nav_state_mirror_matches_documented_layout():
    d = _defines()
    S = _abi.LrlNavState
    assert C.sizeof(S) == d["LRL_NAV_STATE_BYTES"]
    assert S.ids.offset == d["LRL_NAV_STATE_OFF_IDS"]
    assert S.prev_ll.offset == d["LRL_NAV_STATE_OFF_PREV_LL"]
    assert S.n.offset == d["LRL_NAV_STATE_OFF_N"]
    assert S.base_init_state.offset == d["LRL_NAV_STATE_OFF_BASE_INIT_STATE"]
    assert S.term.offset == d["LRL_NAV_STATE_OFF_TERM"]
    assert S.scale.offset == d["LRL_NAV_STATE_OFF_SCALE"]
    assert S.goal_threshold.offset == d["LRL_NAV_STATE_OFF_GOAL_THRESHOLD"]
    assert _abi.NAV_BLOCK == d["LRL_NAV_BLOCK"]
    assert (_abi.NAV_ONLY_FLAGS, _abi.NAV_ONLY_RESET) == (d["LRL_NAV_ONLY_FLAGS"], d["LRL_NAV_ONLY_RESET"])


def test_nav_state_documented_layout_is_the_compilers(tmp_path):
    fields = [f for f, _ in _abi.LrlNavState._fields_]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){printf("%zu %d", ' \
           'sizeof(lrl_nav_state), (int)LRL_NAV_R_NUM);\n' + \
           "".join(f'printf(" %zu", offsetof(lrl_nav_state, {f}));\n' for f in fields) + "return 0;}\n"
    exe = str(tmp_path / "nav_layout")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == C.sizeof(_abi.LrlNavState) == _defines()["LRL_NAV_STATE_BYTES"]
    assert out[1] == len(_abi.NAV_TERMS)
    assert out[2:] == [getattr(_abi.LrlNavState, f).offset for f in fields]


def test_nav_term_names_are_the_wrappers_rewards():
    from lrl.high_level import HighLevelControlWrapper, reward_scales
    names = [k for k in vars(reward_scales) if not k.startswith("__")]
    assert sorted(names) == sorted(_abi.NAV_TERMS)
    for k in _abi.NAV_TERMS:
        assert hasattr(HighLevelControlWrapper, "_reward_" + k)


def test_native_refuses_a_low_level_env_without_a_sim():
    from fake_ll_env import FakeLowLevelEnv
    from lrl.high_level import HighLevelControlWrapper
    g = golden("high_level.npz")
    T, n = g["rew"].shape
    fake = FakeLowLevelEnv(n, T, 5)
    with pytest.raises(TypeError, match="HistoryWrapper over a LeggedRobotEnv"):
        HighLevelControlWrapper(fake, lambda ob: torch.zeros(n, 12), num_envs=n, device="cpu", native=True)
    assert not fake.reset_log and not fake.commands_log  # refused before the env was touched
    # the default is the host path, bit for bit the reference's
    env = HighLevelControlWrapper(fake, lambda ob: torch.zeros(n, 12), num_envs=n, device="cpu")
    assert env.native is False and type(env.extras) is dict
    for t in range(T):
        obs, rew, reset, extras = env.step(torch.tensor(g["actions"][t]))
        np.testing.assert_array_equal(obs["obs"].numpy(), g["obs"][t])
        np.testing.assert_array_equal(rew.numpy(), g["rew"][t])
        np.testing.assert_array_equal(env.episode_sums["total"].numpy(), g["ep_total"][t])
