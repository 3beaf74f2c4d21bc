"""The eval group's parameter block on the host (lrl/params.py eval_group_params, lrl/config.py eval_variant) and its
ctypes mirror: which differences between cfg and eval_cfg become the eval group's lrl_group_params, which are refused,
and that the struct has the header's layout.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROBOT_FILES
from lrl import _abi
from lrl import config as lcfg
from lrl import params as lparams
from lrl.robot import load_robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**over):
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.terrain.x_offset = 0
    lcfg._apply(cfg, over)
    return cfg


@pytest.fixture(scope="module")
def rob():
    return load_robot(ROBOT_FILES["mc"])


def _pair(rob, base=None, **over):
    base = base or {}
    return lparams.build_params(_cfg(**base), rob), lparams.build_params(_cfg(**dict(base, **over)), rob)


def _val(v):
    return list(v) if isinstance(v, C.Array) else v


def test_equal_cfgs_need_no_eval_group(rob):
    P, Pe = _pair(rob)
    assert lparams.eval_group_params(P, Pe) is None
    # what the env sets per group itself does not count as a difference
    Pe.num_train_envs, Pe.teleport_x_offset_eval, Pe.teleport_x_offset = 7, 3.0, 2.0
    assert lparams.eval_group_params(P, Pe) is None


def test_group_fields_are_the_struct_and_exist_in_the_block():
    names = [f for f, _ in _abi.LrlGroupParams._fields_]
    assert tuple(names) == lparams.GROUP_FIELDS
    assert names == ["randomize_motor_strength", "randomize_kp", "randomize_kd", "motor_strength_range", "kp_range",
                     "kd_range", "dr_span", "push_robots", "push_interval", "push_lo", "push_span", "teleport",
                     "teleport_thresh", "terrain_length", "terrain_width", "terrain_rows", "terrain_cols"]
    block = dict(_abi.LrlEnvParams._fields_)
    for f, t in _abi.LrlGroupParams._fields_:
        assert block[f] is t, f  # same name, same type as the train group's field
    assert "rand_interval" not in names and "teleport_x_offset_eval" not in names


# one cfg key -> the group fields it moves (push_max 0.5 -> 0.8 moves lo and span; a range moves its span too)
ALONE = [
    ({"domain_rand.randomize_motor_strength": False}, {"randomize_motor_strength"}),
    ({"domain_rand.randomize_Kp_factor": True}, {"randomize_kp"}),
    ({"domain_rand.randomize_Kd_factor": True}, {"randomize_kd"}),
    ({"domain_rand.motor_strength_range": [0.7, 1.4]}, {"motor_strength_range", "dr_span"}),
    ({"domain_rand.Kp_factor_range": [0.6, 0.9]}, {"kp_range", "dr_span"}),
    ({"domain_rand.Kd_factor_range": [1.6, 2.1]}, {"kd_range", "dr_span"}),
    ({"domain_rand.push_robots": True}, {"push_robots"}),
    ({"domain_rand.push_interval_s": 0.3}, {"push_interval"}),
    ({"domain_rand.max_push_vel_xy": 0.8}, {"push_lo", "push_span"}),
    ({"terrain.teleport_robots": False}, {"teleport"}),  # (on the trimesh base below, where the switch acts)
    ({"terrain.teleport_thresh": 0.7}, {"teleport_thresh"}),
    ({"terrain.terrain_length": 6.0}, {"terrain_length"}),
    ({"terrain.terrain_width": 7.0}, {"terrain_width"}),
    ({"terrain.num_rows": 4}, {"terrain_rows"}),
    ({"terrain.num_cols": 5}, {"terrain_cols"}),
]


@pytest.mark.parametrize("over,moved", ALONE, ids=[next(iter(o)) for o, _ in ALONE])
def test_each_group_field_alone_is_accepted(rob, over, moved):
    P, Pe = _pair(rob, {"terrain.mesh_type": "trimesh", "terrain.teleport_robots": True}, **over)
    assert P.teleport == 1
    before = bytes(memoryview(P).cast("B"))
    G = lparams.eval_group_params(P, Pe)
    assert isinstance(G, _abi.LrlGroupParams)
    assert bytes(memoryview(P).cast("B")) == before  # the train block is not touched
    assert {f for f in lparams.GROUP_FIELDS if _val(getattr(G, f)) != _val(getattr(P, f))} == moved
    for f in lparams.GROUP_FIELDS:  # the eval group's values are the eval cfg's block's
        assert _val(getattr(G, f)) == _val(getattr(Pe, f)), f


def test_spans_are_the_float32_of_the_double_difference(rob):
    ranges = {"domain_rand.motor_strength_range": [0.1, 0.7], "domain_rand.Kp_factor_range": [0.6, 1.3],
              "domain_rand.Kd_factor_range": [0.7, 2.3], "domain_rand.max_push_vel_xy": 0.3}
    P, Pe = _pair(rob, **ranges)
    G = lparams.eval_group_params(P, Pe)
    for i, k in enumerate(("motor_strength_range", "Kp_factor_range", "Kd_factor_range")):
        lo, hi = ranges["domain_rand." + k]
        want = np.float32(hi - lo)  # the python-float difference, rounded once
        assert np.float32(G.dr_span[i]) == want
        # (not the difference of the rounded ends: these ranges are chosen so that the two differ)
        assert np.float32(np.float32(hi) - np.float32(lo)) != want, k
    assert [np.float32(x) for x in G.motor_strength_range] == [np.float32(0.1), np.float32(0.7)]
    assert np.float32(G.push_lo) == np.float32(-0.3) and np.float32(G.push_span) == np.float32(0.3 - (-0.3))
    for i in range(3):  # as build_params computes the train group's
        assert np.float32(P.dr_span[i]) == np.float32([1.1 - 0.9, 1.3 - 0.8, 1.5 - 0.5][i])


REFUSED = [
    ({"control.stiffness": {"joint": 40.0}}, {"p_gains"}),
    ({"rewards.scales.torques": -0.0004}, {"reward_scale"}),
    ({"domain_rand.rand_interval_s": 2}, {"rand_interval"}),
    ({"noise.add_noise": False}, {"add_noise"}),
    ({"env.observe_command": False, "env.num_observations": 39}, {"observe_command", "num_obs", "noise_vec"}),
]


@pytest.mark.parametrize("over,named", REFUSED, ids=[next(iter(o)) for o, _ in REFUSED])
def test_shared_parameters_stay_refused(rob, over, named):
    # ... also when group fields differ as well: the message names the shared fields and no group field
    P, Pe = _pair(rob, **dict(over, **{"domain_rand.push_robots": True, "domain_rand.motor_strength_range": [0.5, 0.6]}))
    with pytest.raises(NotImplementedError) as ei:
        lparams.eval_group_params(P, Pe)
    msg = str(ei.value)
    for f in named:
        assert repr(f) in msg, (f, msg)
    for f in lparams.GROUP_FIELDS:
        assert f not in msg, (f, msg)


def test_terrain_solver_type_stays_refused(rob):
    mk = lambda **o: lparams.build_params(_cfg(**dict({"terrain.mesh_type": "trimesh"}, **o)), rob, terrain_mesh=1)
    P, Pe = mk(), mk(**{"sim.physx.terrain_solver_type": 1, "terrain.teleport_thresh": 0.9})
    with pytest.raises(NotImplementedError) as ei:
        lparams.eval_group_params(P, Pe)
    assert "'solver_tgs'" in str(ei.value) and "teleport" not in str(ei.value)


def test_eval_variant_copies_and_sets():
    cfg = _cfg()
    n_train = cfg.env.num_envs
    ev = lcfg.eval_variant(cfg, 32, ["domain_rand.friction_range=[0.05,0.06]", "domain_rand.push_robots = True",
                                     "control.stiffness={'joint': 30.0}"])
    assert ev.env.num_envs == 32 and cfg.env.num_envs == n_train != 32
    assert ev.domain_rand.friction_range == [0.05, 0.06] and cfg.domain_rand.friction_range == [0.05, 4.5]
    assert ev.domain_rand.push_robots is True and cfg.domain_rand.push_robots is False
    assert ev.control.stiffness == {"joint": 30.0} and cfg.control.stiffness == {"joint": 20.0}
    ev.rewards.scales.torques = 1.0  # an independent tree
    assert cfg.rewards.scales.torques != 1.0
    ev.terrain._update({"terrain.num_rows": 3})  # the copy's nodes know their paths (play.py's _update)
    assert ev.terrain.num_rows == 3 and cfg.terrain.num_rows != 3
    with pytest.raises(AttributeError, match="frictoin_range"):
        lcfg.eval_variant(cfg, 8, ["domain_rand.frictoin_range=[0, 1]"])
    with pytest.raises(ValueError, match="PATH=VALUE"):
        lcfg.eval_variant(cfg, 8, ["domain_rand.push_robots"])
    with pytest.raises((ValueError, SyntaxError)):
        lcfg.eval_variant(cfg, 8, ["domain_rand.push_robots=__import__('os')"])


def test_group_struct_layout_matches_header(tmp_path):
    """Size and field offsets of lrl_group_params against the ctypes mirror, and lrl_env_params unchanged in size (the
    eval block travels beside it, lrl_sim_set_eval_group)."""
    names = [f for f, _ in _abi.LrlGroupParams._fields_]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){\n' \
           'printf("%zu %zu\\n", sizeof(lrl_group_params), sizeof(lrl_env_params));\n' + \
           "".join(f'printf("%zu\\n", offsetof(lrl_group_params, {f}));\n' for f in names) + "return 0;}\n"
    exe = str(tmp_path / "lrl_group_layout")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(_abi.LrlGroupParams), C.sizeof(_abi.LrlEnvParams)] + \
        [getattr(_abi.LrlGroupParams, f).offset for f in names]


def test_eval_terrain_gets_the_tile_size_its_curriculum_reads():
    """_update_terrain_curriculum reads cfg.terrain.env_length of the group's own cfg: the eval tiles' too."""
    from lrl.terrain import Terrain
    small = {"terrain.mesh_type": "trimesh", "terrain.border_size": 1.0, "terrain.num_rows": 2, "terrain.num_cols": 2}
    cfg, ev = _cfg(**small), _cfg(**dict(small, **{"terrain.terrain_length": 6.0, "terrain.terrain_width": 6.0}))
    Terrain(cfg.terrain, 4, ev.terrain, 3)
    assert (cfg.terrain.env_length, ev.terrain.env_length, ev.terrain.env_width) == (8.0, 6.0, 6.0)
