"""The camera's part of the C ABI (include/lrl.h) against its ctypes mirror (lrl/_abi.py): lrl_camera's layout from a
compiled probe, and every LRL_RENDER_* / LRL_CAM_* constant."""
import ctypes as C
import os
import re
import subprocess

from lrl import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lrl.h")


def test_camera_layout_matches_header(tmp_path):
    fields = [f for f, _ in _abi.LrlCamera._fields_]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){printf("%zu", sizeof(lrl_camera));\n' + \
        "".join(f'printf(" %zu", offsetof(lrl_camera, {f}));\n' for f in fields) + "return 0;}\n"
    exe = str(tmp_path / "lrl_camera_check")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(_abi.LrlCamera)] + [getattr(_abi.LrlCamera, f).offset for f in fields]
    assert C.sizeof(_abi.LrlCamera) == 44


def test_render_constants_match_header():
    src = open(HDR).read()
    d = {k: v for k, v in re.findall(r"#define\s+(LRL_(?:RENDER|CAM)_[A-Z_]+)\s+(\S+)", src)}
    num = lambda k: float(d[k].rstrip("fu")) if not d[k].startswith("0x") else int(d[k], 16)
    assert num("LRL_CAM_FOLLOW") == _abi.CAM_FOLLOW
    assert num("LRL_RENDER_ID_SHADOW") == _abi.RENDER_ID_SHADOW
    assert num("LRL_RENDER_LINK_RADIUS") == _abi.RENDER_LINK_RADIUS
    assert num("LRL_RENDER_AMBIENT") == _abi.RENDER_AMBIENT
    assert tuple(num("LRL_RENDER_LIGHT_" + c) for c in "XYZ") == _abi.RENDER_LIGHT
    for name in ("SKY", "GROUND_A", "GROUND_B", "BASE", "SPHERE", "LINK"):
        assert tuple(num(f"LRL_RENDER_{name}_{c}") for c in "RGB") == getattr(_abi, "RENDER_" + name), name
    assert len(d) == 2 + 1 + 1 + 3 + 6 * 3  # nothing in the header is left unmirrored
