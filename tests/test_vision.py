"""lrl.vision without a GPU: the torch form of DepthEncoder against the fp64 restatement (tests/vision_ref.py), its flat
parameter buffer, lrl_vision_net_init's envelope through liblrl.so (a host-only call), the lrl_vision_net mirror's
layout against a compiled probe, and DepthDistiller's rings on a stub env."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
from torch import nn

import vision_ref as vr
from lrl import _abi
from lrl import vision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lrl.h")
VHDR = os.path.join(ROOT, "include", "lrl_vision.h")


def _params(enc):
    return {k: v.detach().double().numpy() for k, v in enc.state_dict().items()}


@pytest.mark.parametrize("h, w, extra, hidden, out", [(16, 24, 5, 16, 18), (48, 64, 0, 128, 7), (8, 8, 2, 24, 3)])
def test_torch_form_matches_the_restatement(h, w, extra, hidden, out):
    torch.manual_seed(h + extra)
    enc = vision.DepthEncoder(h, w, out, extra_dim=extra, hidden=hidden, far=2.5).double()
    assert enc.flat.dtype == torch.float64 and enc.features == h * w // 2
    g = torch.Generator().manual_seed(1)
    img = torch.rand(3, h, w, generator=g, dtype=torch.float64) * 2.5
    ex = torch.randn(3, extra, generator=g, dtype=torch.float64) if extra else None
    tg = torch.randn(3, out, generator=g, dtype=torch.float64)
    enc.zero_grad()
    pred = enc(img, ex)
    loss = torch.nn.functional.mse_loss(pred, tg)
    loss.backward()
    rl, rg, r = vr.mse_grads(_params(enc), img.numpy(), None if ex is None else ex.numpy(), tg.numpy(), 1 / 2.5)
    assert np.allclose(enc.conv_features(img).detach().numpy(), r["features"], rtol=1e-12, atol=1e-14)
    assert np.allclose(pred.detach().numpy(), r["pred"], rtol=1e-12, atol=1e-14)
    assert abs(loss.item() - rl) <= 1e-13 * rl
    for k, p in enc.named_parameters():
        assert np.allclose(p.grad.numpy(), rg[k], rtol=1e-10, atol=1e-14), k
        off, shape = enc.offsets[k]
        assert torch.equal(enc.flat_grad[off:off + p.numel()].view(shape), p.grad)  # the flat gradient holds it


def test_parameters_are_aligned_views_of_one_buffer():
    enc = vision.DepthEncoder(48, 64, 187, extra_dim=42, hidden=128)
    assert [k for k, _ in enc.named_parameters()] == list(vr.KEYS) == list(enc.state_dict())
    end = 0
    for k, p in enc.named_parameters():
        off, shape = enc.offsets[k]
        assert off % 64 == 0 and off >= end and off - end < 64, k
        assert p.data_ptr() == enc.flat.data_ptr() + 4 * off and tuple(p.shape) == shape and p.is_contiguous()
        assert p.grad.data_ptr() == enc.flat_grad.data_ptr() + 4 * off
        end = off + p.numel()
    assert enc.flat.numel() == (end + 63) // 64 * 64 and enc.flat.grad is enc.flat_grad
    with torch.no_grad():
        enc.flat.mul_(2.0)  # writing the buffer writes the parameters
    assert torch.equal(enc.fc2.bias, enc.flat[enc.offsets["fc2.bias"][0]:][:187])
    # an optimiser that drops the gradients does not detach them for good
    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    assert enc.conv1.weight.grad is None
    enc.zero_grad()
    assert enc.conv1.weight.grad.data_ptr() == enc.flat_grad.data_ptr()


def test_state_dict_round_trips_with_a_plain_torch_module():
    class Plain(nn.Module):
        def __init__(self, h, w, out, extra, hidden):
            super().__init__()
            self.conv1 = nn.Conv2d(1, 16, 5, stride=2, padding=2)
            self.conv2 = nn.Conv2d(16, 32, 3, stride=2, padding=1)
            self.conv3 = nn.Conv2d(32, 32, 3, stride=2, padding=1)
            self.fc1 = nn.Linear(h * w // 2 + extra, hidden)
            self.fc2 = nn.Linear(hidden, out)

        def forward(self, img, ex):
            x = img.unsqueeze(1) / 3.0
            for c in (self.conv1, self.conv2, self.conv3):
                x = nn.functional.elu(c(x))
            return self.fc2(nn.functional.elu(self.fc1(torch.cat([x.flatten(1), ex], 1))))

    torch.manual_seed(3)
    plain, enc = Plain(16, 24, 9, 4, 32), vision.DepthEncoder(16, 24, 9, extra_dim=4, hidden=32, far=3.0)
    enc.load_state_dict(plain.state_dict(), strict=True)
    ptr = enc.flat.data_ptr()
    assert enc.conv2.weight.data_ptr() == ptr + 4 * enc.offsets["conv2.weight"][0]  # loaded in place
    img, ex = torch.rand(2, 16, 24) * 3, torch.randn(2, 4)
    assert torch.allclose(enc(img, ex), plain(img, ex), rtol=1e-5, atol=1e-6)
    other = Plain(16, 24, 9, 4, 32)
    other.load_state_dict(enc.state_dict(), strict=True)
    for k, v in plain.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k


def _init(h, w, extra, hidden, out, scale=1 / 3.0):
    n = vision.LrlVisionNet()
    rc = vision.lib().lrl_vision_net_init(C.addressof(n), h, w, extra, hidden, out, scale)
    return rc, n, (vision.lib().lrl_last_error() or b"").decode()


@pytest.mark.parametrize("h, w, extra, hidden, out", [(16, 16, 0, 16, 1), (48, 64, 256, 256, 256), (16, 192, 0, 16, 256),
                                                      (192, 16, 256, 256, 1), (24, 128, 5, 128, 187)])
def test_net_init_accepts_the_envelope_and_lays_the_fields_out(h, w, extra, hidden, out):
    rc, n, _ = _init(h, w, extra, hidden, out)
    assert rc == 0
    assert (n.height, n.width, n.extra, n.hidden, n.out, n.features) == (h, w, extra, hidden, out, h * w // 2)
    assert n.ld_x >= n.features + extra and n.ld_x % 4 == 0 and abs(n.input_scale - 1 / 3.0) < 1e-7
    offs, total = vision.field_offsets(h, w, extra, hidden, out)
    assert {k: getattr(n, f) for k, f in vision._FIELDS} == {k: o for k, (o, _) in offs.items()}
    assert n.total == total
    assert vision.in_envelope(h, w, extra, hidden, out)
    assert vision.lib().lrl_vision_workspace_bytes(C.addressof(n), 3) > 0


@pytest.mark.parametrize("args, names", [
    ((8, 64, 0, 16, 1), "height"), ((20, 64, 0, 16, 1), "height"), ((48, 8, 0, 16, 1), "width"),
    ((48, 60, 0, 16, 1), "width"), ((48, 72, 0, 16, 1), r"height \* width"), ((56, 56, 0, 16, 1), r"height \* width"),
    ((16, 16, -1, 16, 1), "extra"), ((16, 16, 257, 16, 1), "extra"), ((16, 16, 0, 0, 1), "hidden"),
    ((16, 16, 0, 24, 1), "hidden"), ((16, 16, 0, 272, 1), "hidden"), ((16, 16, 0, 16, 0), "out"),
    ((16, 16, 0, 16, 257), "out"),
])
def test_net_init_refuses_each_violated_bound_by_name(args, names):
    rc, n, msg = _init(*args)
    assert rc == -1 and re.search(names, msg), msg  # LRL_E_INVALID
    assert n.total == 0  # the descriptor is left as it was
    assert not vision.in_envelope(*args)
    assert vision.lib().lrl_vision_workspace_bytes(C.addressof(n), 3) == 0
    # the module then keeps to its torch form
    h, w, extra, hidden, out = args
    if extra >= 0 and hidden > 0 and out > 0 and h % 8 == 0 and w % 8 == 0:
        enc = vision.DepthEncoder(h, w, out, extra_dim=extra, hidden=hidden)
        assert not enc.native_ok
        assert enc(torch.rand(2, h, w), torch.zeros(2, extra)).shape == (2, out)
        with pytest.raises(RuntimeError, match="envelope"):
            enc.forward_native(torch.rand(2, h, w))


def test_vision_net_layout_matches_header(tmp_path):
    fields = [f for f, _ in vision.LrlVisionNet._fields_]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){printf("%zu", sizeof(lrl_vision_net));\n' + \
        "".join(f'printf(" %zu", offsetof(lrl_vision_net, {f}));\n' for f in fields) + \
        'printf(" %d", LRL_VISION_MAX_WORKGROUPS);\nreturn 0;}\n'
    exe = str(tmp_path / "lrl_vision_net_check")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(vision.LrlVisionNet)] + [getattr(vision.LrlVisionNet, f).offset for f in fields] + \
        [vision.MAX_WORKGROUPS]
    assert C.sizeof(vision.LrlVisionNet) == 120
    assert "lrl_vision_net" not in _abi.MIRRORS  # the entry points take its address as a plain pointer
    src = open(HDR).read()
    assert re.search(r"#define\s+LRL_ABI_VERSION\s+6\b", src)
    sig = _abi.signatures(open(VHDR).read())
    assert "lrl_vision.h" in src and not re.search(r"lrl_vision_\w+\s*\(", src)  # lrl.h includes it, declares none
    for name in ("lrl_vision_net_init", "lrl_vision_workspace_bytes", "lrl_vision_forward", "lrl_vision_forward_backward"):
        assert sig[name][1][0] is C.c_void_p, name
    assert sig["lrl_vision_workspace_bytes"][0] is C.c_int64


def _stub_env(n=6, first=5, scan=4, h=16, w=16):
    cfg = types.SimpleNamespace(env=types.SimpleNamespace(num_height_points=scan, num_observations=first + scan),
                                terrain=types.SimpleNamespace(measure_heights=True))
    return types.SimpleNamespace(cfg=cfg, depth_images=torch.zeros(n, h, w), num_envs=n)


def test_distiller_rings_wrap_and_split_the_columns():
    torch.manual_seed(0)
    env = _stub_env()
    enc = vision.DepthEncoder(16, 16, 4, extra_dim=5, hidden=16)
    d = vision.DepthDistiller(env, enc, capacity=16, batch_size=8, lr=1e-3)
    assert not d.native and (d.first, d.num_scan) == (5, 4)
    fed_img, fed_obs = [], []
    for step in range(4):  # 24 rows into a ring of 16: the third batch wraps, the oldest rows are overwritten
        env.depth_images = torch.rand(6, 16, 16) * 3
        obs = torch.randn(6, 9)
        d.collect(obs)
        fed_img.append(env.depth_images.clone())
        fed_obs.append(obs.clone())
        assert d.size == min(6 * (step + 1), 16) and d.head == 6 * (step + 1) % 16
    img, obs = torch.cat(fed_img), torch.cat(fed_obs)
    for j in range(24):
        slot = j % 16
        if j >= 24 - 16:  # the newest 16 rows are the ones held
            assert torch.equal(d.images[slot], img[j]) and torch.equal(d.obs[slot], obs[j])
    assert torch.equal(d.extra, d.obs[:, :5]) and torch.equal(d.target, d.obs[:, 5:])
    assert d.extra.data_ptr() == d.obs.data_ptr() and d.target.stride(0) == 9
    with pytest.raises(ValueError, match="do not fit"):
        vision.DepthDistiller(env, enc, capacity=4).collect(obs[:6])
    # the torch path trains: a fixed batch's loss falls
    rows = [torch.arange(16)] * 25
    first = d.update(1, rows=rows[:1]).item()
    d.update(24, rows=rows[1:])
    assert d.update(1, rows=rows[:1]).item() < first


def test_distiller_predict_obs_swaps_the_scan_columns_only():
    torch.manual_seed(1)
    env = _stub_env()
    enc = vision.DepthEncoder(16, 16, 4, extra_dim=5, hidden=16)
    d = vision.DepthDistiller(env, enc, capacity=8)
    env.depth_images = torch.rand(6, 16, 16) * 3
    obs = torch.randn(6, 9)
    keep = obs.clone()
    out = d.predict_obs(obs)
    assert torch.equal(obs, keep) and out.data_ptr() != obs.data_ptr()
    assert torch.equal(out[:, :5], obs[:, :5])
    with torch.no_grad():
        assert torch.equal(out[:, 5:], enc(env.depth_images, obs[:, :5]))
    with pytest.raises(ValueError, match="5 \\+ 4"):
        vision.DepthDistiller(env, vision.DepthEncoder(16, 16, 3, extra_dim=5, hidden=16), capacity=8)
    with pytest.raises(ValueError, match="16 x 16"):
        vision.DepthDistiller(env, vision.DepthEncoder(16, 24, 4, extra_dim=5, hidden=16), capacity=8)


def test_env_depth_refreshed_follows_the_update_interval():
    """The property's arithmetic on the env's own counters (the env itself needs a GPU: tests/test_vision_gpu.py)."""
    from lrl.env import LeggedRobotEnv
    assert isinstance(LeggedRobotEnv.depth_refreshed, property) and LeggedRobotEnv.depth_refreshed.fset is None
    e = types.SimpleNamespace(_depth_cam=None, _depth_step=0, _depth_interval=5)
    get = LeggedRobotEnv.depth_refreshed.fget
    assert get(e) is False
    e._depth_cam = object()
    seen = []
    for step in range(12):  # _depth_tick: a full refresh when the pre-increment count is a multiple of the interval
        seen.append(get(e))
        e._depth_step += 1
    assert seen == [False, True, False, False, False, False, True, False, False, False, False, True]
