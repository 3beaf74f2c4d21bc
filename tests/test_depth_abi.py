"""The depth camera's part of the C ABI (include/lrl.h) against its ctypes mirror (lrl/_abi.py): lrl_depth_camera's
layout from a compiled probe, every LRL_DEPTH_* constant, and the cfg group lrl.config.add_depth_camera installs."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lrl import _abi
from lrl import config as lcfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lrl.h")


def test_depth_camera_layout_matches_header(tmp_path):
    fields = [f for f, _ in _abi.LrlDepthCamera._fields_]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){printf("%zu", sizeof(lrl_depth_camera));\n' + \
        "".join(f'printf(" %zu", offsetof(lrl_depth_camera, {f}));\n' for f in fields) + "return 0;}\n"
    exe = str(tmp_path / "lrl_depth_camera_check")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(_abi.LrlDepthCamera)] + [getattr(_abi.LrlDepthCamera, f).offset for f in fields]
    assert C.sizeof(_abi.LrlDepthCamera) == 40
    assert fields == ["pos", "pitch_deg", "hfov_deg", "near", "far", "width", "height", "flags"]


def test_depth_constants_match_header():
    src = open(HDR).read()
    d = {k: v for k, v in re.findall(r"#define\s+(LRL_DEPTH_[A-Z_]+)\s+(\S+)", src)}
    assert int(d["LRL_DEPTH_NO_ROBOT"].rstrip("u"), 0) == _abi.DEPTH_NO_ROBOT
    assert len(d) == 1  # nothing in the header is left unmirrored
    # the entry point is declared, and the ABI version did not move for it (an appended entry point)
    assert re.search(r"int32_t\s+lrl_sim_depth\s*\(", src)
    assert re.search(r"#define\s+LRL_ABI_VERSION\s+6\b", src)


def test_add_depth_camera_defaults_and_overrides():
    cfg = lcfg.make_cfg()
    assert not hasattr(cfg, "depth") and not hasattr(lcfg.Cfg, "depth") and "depth" not in cfg.to_dict()
    out = lcfg.add_depth_camera(cfg)
    assert out is cfg
    assert cfg.depth.to_dict() == dict(width=64, height=48, hfov_deg=87.0, pos=[0.27, 0.0, 0.03], pitch_deg=20.0,
                                       near=0.05, far=3.0, update_interval=5, see_robot=True)
    other = lcfg.make_cfg()
    lcfg.add_depth_camera(other, width=32, far=5.0, see_robot=False, pos=[0.3, 0.0, 0.1])
    assert (other.depth.width, other.depth.height, other.depth.far, other.depth.see_robot) == (32, 48, 5.0, False)
    assert other.depth.pos == [0.3, 0.0, 0.1]
    other.depth.pos[0] = 9.0  # (each cfg owns its lists)
    assert cfg.depth.pos == [0.27, 0.0, 0.03] and lcfg.add_depth_camera(lcfg.make_cfg()).depth.pos[0] == 0.27
    assert not hasattr(lcfg.make_cfg(), "depth")  # installing it on one tree leaves the defaults alone
    with pytest.raises(KeyError, match="fov"):
        lcfg.add_depth_camera(lcfg.make_cfg(), fov=90.0)
    # the group follows the tree's _update convention (plain or prefixed keys)
    cfg.depth._update({"depth.update_interval": 2, "terrain.width": 7})
    assert cfg.depth.update_interval == 2 and cfg.depth.width == 64


@pytest.mark.parametrize("native", [False, True])
def test_navigation_wrapper_refuses_a_low_level_env_with_the_sensor(native):
    """The wrapper resets the low-level envs after their step's depth refresh: it names the key and raises, on both of
    its paths, before it touches the env."""
    import types
    from lrl.high_level import HighLevelControlWrapper
    cfg = lcfg.add_depth_camera(lcfg.config_go1(lcfg.make_cfg()))
    ll_env = types.SimpleNamespace(env=types.SimpleNamespace(cfg=cfg), device="cpu", num_envs=4)
    with pytest.raises(ValueError, match=r"Cfg\.depth"):
        HighLevelControlWrapper(ll_env, lambda ob: None, native=native)


def test_preset_cfgs_have_no_depth_group():
    for preset in (lcfg.config_mini_cheetah, lcfg.config_go1):
        cfg = preset(lcfg.make_cfg())
        assert not hasattr(cfg, "depth") and "depth" not in vars(cfg)
