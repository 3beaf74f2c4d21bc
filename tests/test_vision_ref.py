"""tests/vision_ref.py (the fp64 restatement the depth encoder's tests compare with) on cases worked by hand and
against torch.nn.functional.conv2d with autograd in fp64."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import vision_ref as vr


def test_delta_image_reads_the_kernel_flipped():
    """One lit pixel at (4, 6), stride 1: the output around it is the kernel mirrored in both axes (cross-correlation)."""
    x = np.zeros((1, 1, 9, 11))
    x[0, 0, 4, 6] = 1.0
    w = np.arange(1.0, 10.0).reshape(1, 1, 3, 3)
    out = vr.conv2d(x, w, np.zeros(1), 1, 1)
    assert out.shape == (1, 1, 9, 11)
    assert np.array_equal(out[0, 0, 3:6, 5:8], w[0, 0, ::-1, ::-1])
    assert out.sum() == w.sum()


def test_one_hot_kernel_samples_the_strided_shifted_input():
    """A kernel that is 1 at tap (ky, kx) of channel c: out[y, x] = xpad[c, 2 y + ky, 2 x + kx]."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 8, 16))
    for c, ky, kx in ((0, 0, 0), (1, 4, 2), (2, 2, 4), (1, 3, 1)):
        w = np.zeros((1, 3, 5, 5))
        w[0, c, ky, kx] = 1.0
        out = vr.conv2d(x, w, np.array([0.25]), 2, 2)
        xp = np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2)))
        assert out.shape == (2, 1, 4, 8)
        assert np.array_equal(out[:, 0], xp[:, c, ky:ky + 8:2, kx:kx + 16:2] + 0.25)


@pytest.mark.parametrize("pixel, hits", [
    ((0, 3), {(0, 1): (1, 2), (0, 2): (1, 0)}),      # top row: kernel row 1 only (row 0 looks at the padding above)
    ((7, 3), {(3, 1): (2, 2), (3, 2): (2, 0)}),      # bottom row: seen by output row 3 through kernel row 2 only
    ((3, 0), {(1, 0): (2, 1), (2, 0): (0, 1)}),      # left column
    ((3, 7), {(1, 3): (2, 2), (2, 3): (0, 2)}),      # right column: output column 3, kernel column 2
])
def test_border_pixels_of_a_3x3_stride_2_pad_1_layer(pixel, hits):
    """One lit border pixel of an 8 x 8 image: the outputs that see it and the tap each sees it through, by hand
    (input row i is read by output row y through kernel row ky = i + 1 - 2 y)."""
    x = np.zeros((1, 1, 8, 8))
    x[0, 0, pixel[0], pixel[1]] = 1.0
    w = np.arange(1.0, 10.0).reshape(1, 1, 3, 3)
    out = vr.conv2d(x, w, np.zeros(1), 2, 1)[0, 0]
    want = np.zeros((4, 4))
    for (y, xo), (ky, kx) in hits.items():
        want[y, xo] = w[0, 0, ky, kx]
    assert np.array_equal(out, want)


def test_elu_and_its_gradient_from_the_output():
    x = np.array([-30.0, -1.0, -1e-9, 0.0, 1e-9, 2.0])
    y = vr.elu(x)
    assert np.allclose(y, np.where(x > 0, x, np.exp(x) - 1), rtol=0, atol=1e-16)
    # (y + 1 rounds at the scale of 1: an absolute error of one fp64 epsilon, whatever exp(x) is)
    assert np.allclose(vr.elu_grad_from_output(y), np.where(x > 0, 1.0, np.exp(x)), rtol=0, atol=2.3e-16)


@pytest.mark.parametrize("cin, cout, k, stride, pad, h, w", [(1, 16, 5, 2, 2, 16, 24), (16, 32, 3, 2, 1, 8, 12),
                                                              (3, 4, 3, 1, 1, 5, 7), (2, 3, 5, 2, 2, 7, 9)])
def test_conv_and_its_gradients_against_torch_fp64(cin, cout, k, stride, pad, h, w):
    rng = np.random.default_rng(k * 100 + h)
    x, wt, b = rng.standard_normal((3, cin, h, w)), rng.standard_normal((cout, cin, k, k)), rng.standard_normal(cout)
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, wt, b))
    tout = F.conv2d(tx, tw, tb, stride=stride, padding=pad)
    out = vr.conv2d(x, wt, b, stride, pad)
    assert out.shape == tuple(tout.shape)
    assert np.allclose(out, tout.detach().numpy(), rtol=1e-13, atol=1e-13)
    gout = rng.standard_normal(out.shape)
    (tout * torch.tensor(gout)).sum().backward()
    dx, dw, db = vr.conv2d_grads(x, wt, gout, stride, pad)
    for mine, ref in ((dx, tx.grad), (dw, tw.grad), (db, tb.grad)):
        assert np.allclose(mine, ref.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("h, w, extra, hidden, out", [(16, 24, 5, 16, 18), (16, 16, 0, 32, 1)])
def test_whole_network_and_mse_gradients_against_torch_fp64(h, w, extra, hidden, out):
    rng = np.random.default_rng(h + w + extra)
    feat = 32 * (h // 8) * (w // 8)
    shapes = {"conv1.weight": (16, 1, 5, 5), "conv1.bias": (16,), "conv2.weight": (32, 16, 3, 3), "conv2.bias": (32,),
              "conv3.weight": (32, 32, 3, 3), "conv3.bias": (32,), "fc1.weight": (hidden, feat + extra),
              "fc1.bias": (hidden,), "fc2.weight": (out, hidden), "fc2.bias": (out,)}
    assert tuple(shapes) == vr.KEYS
    P = {k: rng.standard_normal(s) * 0.2 for k, s in shapes.items()}
    img, ex, tg = rng.random((4, h, w)) * 3.0, rng.standard_normal((4, extra)), rng.standard_normal((4, out))
    T = {k: torch.tensor(v, requires_grad=True) for k, v in P.items()}
    a = torch.tensor(img)[:, None] * (1 / 3.0)
    for name, pad in (("conv1", 2), ("conv2", 1), ("conv3", 1)):
        a = F.elu(F.conv2d(a, T[name + ".weight"], T[name + ".bias"], stride=2, padding=pad))
    feats = a.flatten(1)
    pred = F.linear(F.elu(F.linear(torch.cat([feats, torch.tensor(ex)], 1), T["fc1.weight"], T["fc1.bias"])),
                    T["fc2.weight"], T["fc2.bias"])
    tloss = F.mse_loss(pred, torch.tensor(tg))
    tloss.backward()
    loss, g, r = vr.mse_grads(P, img, ex if extra else None, tg, 1 / 3.0)
    assert r["features"].shape == (4, h * w // 2)
    assert np.allclose(r["features"], feats.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(r["pred"], pred.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert abs(loss - tloss.item()) <= 1e-13 * abs(loss)
    for k in vr.KEYS:
        assert np.allclose(g[k], T[k].grad.numpy(), rtol=1e-10, atol=1e-13), k
