"""fp64 numpy restatement of the depth encoder (include/lrl_vision.h) and of its MSE gradients, for the
tests: explicit sums over the kernel taps of zero-padded arrays, no call into lrl.vision or torch.

params: {state_dict key: array} with conv1.weight [16,1,5,5], conv2.weight [32,16,3,3], conv3.weight [32,32,3,3],
fc1.weight [hidden, F + E], fc2.weight [out, hidden] and their biases.
"""
import numpy as np

LAYERS = (("conv1", 2, 2), ("conv2", 2, 1), ("conv3", 2, 1))  # name, stride, pad
KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight",
        "fc1.bias", "fc2.weight", "fc2.bias")


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def elu_grad_from_output(y):
    """elu'(x) written with y = elu(x): 1 for y > 0, y + 1 (= exp(x)) otherwise."""
    return np.where(y > 0, 1.0, y + 1.0)


def _padded(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))


def _taps(xp, k, stride, ho, wo):
    """(ky, kx, the [N, C, ho, wo] slice of the padded input that tap multiplies)"""
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, xp[:, :, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride]


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv2d(x, w, b, stride, pad):
    """torch cross-correlation: out[n, o, y, x] = b[o] + sum_{c, ky, kx} xpad[n, c, s y + ky, s x + kx] w[o, c, ky, kx]"""
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    k = w.shape[2]
    ho, wo = out_size(x.shape[2], k, stride, pad), out_size(x.shape[3], k, stride, pad)
    out = np.zeros((x.shape[0], w.shape[0], ho, wo)) + b[None, :, None, None]
    for ky, kx, xs in _taps(_padded(x, pad), k, stride, ho, wo):
        out += np.einsum("ncyx,oc->noyx", xs, w[:, :, ky, kx])
    return out


def conv2d_grads(x, w, gout, stride, pad):
    """(d/dx, d/dw, d/db) of sum(out * gout) for out = conv2d(x, w, b, stride, pad)"""
    x, w, gout = (np.asarray(a, np.float64) for a in (x, w, gout))
    k = w.shape[2]
    ho, wo = gout.shape[2:]
    xp = _padded(x, pad)
    dxp, dw = np.zeros_like(xp), np.zeros_like(w)
    for ky, kx, xs in _taps(xp, k, stride, ho, wo):
        dw[:, :, ky, kx] = np.einsum("noyx,ncyx->oc", gout, xs)
        dxp[:, :, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride] += np.einsum("noyx,oc->ncyx", gout,
                                                                                      w[:, :, ky, kx])
    h, wd = x.shape[2:]
    return dxp[:, :, pad:pad + h, pad:pad + wd], dw, gout.sum((0, 2, 3))


def forward(params, images, extra, input_scale):
    """Every intermediate: x0 (scaled input), a1..a3 (ELU outputs), features, xcat, h, pred."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    r = {"x0": np.asarray(images, np.float64)[:, None] * float(input_scale)}
    a = r["x0"]
    for i, (name, stride, pad) in enumerate(LAYERS, 1):
        a = r[f"a{i}"] = elu(conv2d(a, P[name + ".weight"], P[name + ".bias"], stride, pad))
    r["features"] = a.reshape(a.shape[0], -1)
    e = np.zeros((a.shape[0], 0)) if extra is None else np.asarray(extra, np.float64)
    r["xcat"] = np.concatenate([r["features"], e], 1)
    r["h"] = elu(r["xcat"] @ P["fc1.weight"].T + P["fc1.bias"])
    r["pred"] = r["h"] @ P["fc2.weight"].T + P["fc2.bias"]
    return r


def mse_grads(params, images, extra, target, input_scale):
    """(loss, {key: gradient}, forward dict) of loss = mean((pred - target)^2)"""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    r = forward(P, images, extra, input_scale)
    diff = r["pred"] - np.asarray(target, np.float64)
    loss = float(np.mean(diff * diff))
    g = {}
    dpred = 2.0 * diff / diff.size
    g["fc2.weight"], g["fc2.bias"] = dpred.T @ r["h"], dpred.sum(0)
    dh = (dpred @ P["fc2.weight"]) * elu_grad_from_output(r["h"])
    g["fc1.weight"], g["fc1.bias"] = dh.T @ r["xcat"], dh.sum(0)
    nf = r["features"].shape[1]
    da = (dh @ P["fc1.weight"][:, :nf]).reshape(r["a3"].shape)
    inputs = [r["x0"], r["a1"], r["a2"]]
    for i in (3, 2, 1):
        name, stride, pad = LAYERS[i - 1]
        gz = da * elu_grad_from_output(r[f"a{i}"])
        da, g[name + ".weight"], g[name + ".bias"] = conv2d_grads(inputs[i - 1], P[name + ".weight"], gz, stride, pad)
    r["d_pred"] = dpred
    return loss, g, r
