"""The depth sensor model's part of the C ABI (include/lrl.h) against its ctypes mirror (lrl/_abi.py):
lrl_depth_sensor's layout from a compiled probe, the LRL_SENSE_* and LRL_RNG_DEPTH enums, and the cfg group
lrl.config.add_depth_sensor installs."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lrl import _abi
from lrl import config as lcfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FIELDS = ["width", "height", "near", "far", "noise_a", "noise_b", "dropout_p", "edge_thresh", "invalid_value", "quant",
          "latency_min", "latency_max"]


def _probe(tmp_path, body, name):
    exe = str(tmp_path / name)
    with open(exe + ".c", "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\n#include "lrl_philox.h"\nint main(){\n' + body +
                "return 0;}\n")
    subprocess.check_call(["gcc", "-I", INC, "-o", exe, exe + ".c"])
    return [int(x) for x in subprocess.check_output([exe]).split()]


def test_depth_sensor_layout_matches_header(tmp_path):
    fields = [f for f, _ in _abi.LrlDepthSensor._fields_]
    assert fields == FIELDS
    body = 'printf("%zu", sizeof(lrl_depth_sensor));\n' + \
        "".join(f'printf(" %zu", offsetof(lrl_depth_sensor, {f}));\n' for f in fields)
    out = _probe(tmp_path, body, "lrl_depth_sensor_check")
    assert out == [C.sizeof(_abi.LrlDepthSensor)] + [getattr(_abi.LrlDepthSensor, f).offset for f in fields]
    assert out == [48] + [4 * k for k in range(12)]
    kinds = {f: t for f, t in _abi.LrlDepthSensor._fields_}
    assert all(kinds[f] is C.c_int32 for f in ("width", "height", "latency_min", "latency_max"))
    assert all(kinds[f] is C.c_float for f in FIELDS[2:10])


def test_enums_match_header(tmp_path):
    out = _probe(tmp_path, 'printf("%d %d %d %d %d", LRL_SENSE_PUSH, LRL_SENSE_RESET_ONLY, LRL_SENSE_FILL, '
                           'LRL_RNG_DEPTH, LRL_RNG_TERRAIN);\n', "lrl_sense_enum_check")
    assert out == [_abi.SENSE_PUSH, _abi.SENSE_RESET_ONLY, _abi.SENSE_FILL, _abi.RNG_DEPTH, 7]
    assert out[:4] == [0, 1, 2, 8]  # the stream is appended: the earlier ones keep their ids


def test_entry_point_is_declared_and_the_header_keeps_its_pins():
    src = open(os.path.join(INC, "lrl.h")).read()
    sense = open(os.path.join(INC, "lrl_depth_sense.h")).read()
    assert list(_abi.signatures(sense)) == ["lrl_sim_depth_sense"]
    sig = _abi.signatures(sense)["lrl_sim_depth_sense"]
    vp, i32 = C.c_void_p, C.c_int32
    assert sig == (C.c_int32, [vp, vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp])
    # lrl.h includes the header and declares nothing of it itself; the loader types the entry point from it
    assert '#include "lrl_depth_sense.h"' in src and not re.search(r"lrl_sim_depth_sense\s*\(", src)
    assert "lrl_depth_sensor" not in _abi.MIRRORS  # the entry point takes byref(LrlDepthSensor) as a plain pointer
    fn = _abi.lib().lrl_sim_depth_sense
    assert (fn.restype, fn.argtypes) == sig
    # an appended entry point: the ABI version stays, and the camera's one LRL_DEPTH_* define stays the only one
    assert re.search(r"#define\s+LRL_ABI_VERSION\s+6\b", src)
    assert re.findall(r"#define\s+(LRL_DEPTH_[A-Z_]+)", src) == ["LRL_DEPTH_NO_ROBOT"]


def test_add_depth_sensor_defaults_and_overrides():
    cfg = lcfg.make_cfg()
    assert not hasattr(cfg, "depth_sensor") and not hasattr(lcfg.Cfg, "depth_sensor")
    assert "depth_sensor" not in cfg.to_dict()
    out = lcfg.add_depth_sensor(cfg)
    assert out is cfg
    assert cfg.depth_sensor.to_dict() == dict(noise_a=0.001, noise_b=0.005, dropout_p=0.01, edge_thresh=0.1,
                                              invalid_value=None, quant=0.001, latency_frames=[0, 1])
    assert not hasattr(cfg, "depth")  # a group of its own: it neither installs nor touches the camera's
    lcfg.add_depth_camera(cfg)
    assert len(cfg.depth.to_dict()) == 9 and "noise_a" not in cfg.depth.to_dict()
    other = lcfg.add_depth_sensor(lcfg.make_cfg(), noise_b=0.0, invalid_value=0.0, latency_frames=(2, 3))
    assert (other.depth_sensor.noise_b, other.depth_sensor.invalid_value, other.depth_sensor.noise_a) == (0.0, 0.0, 0.001)
    assert other.depth_sensor.latency_frames == [2, 3]
    other.depth_sensor.latency_frames[0] = 9  # (each cfg owns its lists)
    assert cfg.depth_sensor.latency_frames == [0, 1]
    assert lcfg.add_depth_sensor(lcfg.make_cfg()).depth_sensor.latency_frames == [0, 1]
    assert not hasattr(lcfg.make_cfg(), "depth_sensor")
    with pytest.raises(KeyError, match="sigma"):
        lcfg.add_depth_sensor(lcfg.make_cfg(), sigma=0.1)
    cfg.depth_sensor._update({"depth_sensor.quant": 0.0, "depth.width": 7})
    assert cfg.depth_sensor.quant == 0.0 and cfg.depth.width == 64


def test_preset_cfgs_have_no_depth_sensor_group():
    for preset in (lcfg.config_mini_cheetah, lcfg.config_go1):
        cfg = preset(lcfg.make_cfg())
        assert not hasattr(cfg, "depth_sensor") and "depth_sensor" not in vars(cfg)
