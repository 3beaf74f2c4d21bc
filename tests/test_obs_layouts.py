"""Parameter block of the observation-layout switches (env.observe_only_ang_vel / observe_only_lin_vel / observe_yaw,
commands.global_reference) against the reference's fixtures (tests/golden/make_golden_obs.py)."""
import ctypes as C

import numpy as np
import pytest

from helpers import golden, make
from lrl import _abi
from obs_layouts import CASES, SWITCHES

NEW = list(SWITCHES)
OFF = _abi.LrlEnvParams.observe_only_ang_vel.offset  # the first of the four appended fields


def _bytes(P):
    return bytes(memoryview(P).cast("B"))


@pytest.mark.parametrize("case", list(CASES))
def test_build_params_layouts(case):
    robot, fixture, over = CASES[case]
    g = golden(fixture)
    cfg, _, _, P = make(robot, **over)
    n_obs = over["env.num_observations"]
    assert P.num_obs == n_obs == g["obs"].shape[2]
    if over.get("noise.add_noise", True):
        assert P.add_noise == 1
        np.testing.assert_array_equal(np.array(P.noise_vec[:n_obs], np.float32), g["noise_scale_vec"])
    else:
        assert P.add_noise == 0
    for f, key in SWITCHES.items():
        assert getattr(P, f) == int(bool(over.get(key, False))), f


def test_only_ang_vel_with_noise_is_refused_like_the_reference():
    with pytest.raises(RuntimeError, match=r"\(45\).*\(42\)"):
        make("mc", **{"env.observe_only_ang_vel": True, "env.num_observations": 45})
    make("mc", **{"env.observe_only_ang_vel": True, "env.num_observations": 45, "noise.add_noise": False})


@pytest.mark.parametrize("over", [{"env.observe_only_lin_vel": True}, {"env.observe_yaw": True, "env.num_observations": 42},
                                  {"env.observe_only_ang_vel": True, "noise.add_noise": False,
                                   "env.num_observations": 44}])
def test_wrong_num_observations_still_raises(over):
    with pytest.raises(ValueError, match="num_observations"):
        make("mc", **over)


@pytest.mark.parametrize("robot", ["mc", "go1"])
def test_switches_off_leave_the_block_unchanged(robot):
    P, P2 = make(robot)[3], make(robot)[3]
    a = _bytes(P)
    assert C.sizeof(P) == OFF + 4 * len(NEW) and len(a) == C.sizeof(P)
    assert a[:OFF] == _bytes(P2)[:OFF]
    assert a[OFF:] == bytes(4 * len(NEW))  # all four fields zero: the layout and reward of before
    # a switch moves only its own field and the layout's size / noise entries
    Pl = make(robot, **{"env.observe_only_lin_vel": True, "env.num_observations": 45})[3]
    T = _abi.LrlEnvParams
    span = lambda Q, f: _bytes(Q)[getattr(T, f).offset:getattr(T, f).offset + getattr(T, f).size]
    assert {f for f, _ in T._fields_ if span(P, f) != span(Pl, f)} == {"num_obs", "noise_vec", "observe_only_lin_vel"}
    Pg = make(robot, **{"commands.global_reference": True})[3]
    assert _bytes(Pg)[:OFF] == a[:OFF] and Pg.global_reference == 1
