"""A numpy restatement of the depth sensor model (include/lrl.h: lrl_sim_depth_sense), independent of the product:
uniforms from aux_ref's Philox, masks (far, edge loss, dropout) and the ring's bookkeeping in exact float32 / integer
arithmetic, values in float64 from the float32 uniforms (``dtype=np.float32``: every line rounded to float32 as the
header writes it; its normal is the float64 one rounded once, so it is bit-exact with a kernel only where sigma is 0).
tests/test_depth_sensor_ref.py pins it on hand cases; tests/test_depth_sensor_gpu.py judges the kernel against it.
"""
import types

import numpy as np

import aux_ref as ar

F32 = np.float32
RNG_DEPTH = 8  # LRL_RNG_DEPTH (include/lrl_philox.h)
PUSH, RESET_ONLY, FILL = 0, 1, 2
LATENCY_PIXEL = 0xFFFFFFFF  # the Philox block index of the delay's draw: no pixel has it


def params(width, height, near=0.05, far=3.0, noise_a=0.0, noise_b=0.0, dropout_p=0.0, edge_thresh=0.0,
           invalid_value=None, quant=0.0, latency=(0, 0)):
    """lrl_depth_sensor with every float rounded to float32, as the struct holds it."""
    return types.SimpleNamespace(
        width=int(width), height=int(height), near=F32(near), far=F32(far), noise_a=F32(noise_a), noise_b=F32(noise_b),
        dropout_p=F32(dropout_p), edge_thresh=F32(edge_thresh),
        invalid_value=F32(far if invalid_value is None else invalid_value), quant=F32(quant),
        latency_min=int(latency[0]), latency_max=int(latency[1]))


def pixel_uniforms(genv, frame, seed, npx):
    """u0, u1, u2 of pixels 0 .. npx - 1: words 0..2 of block px on stream RNG_DEPTH.  float32 [npx, 3]."""
    c1, c2 = ar.step_key(RNG_DEPTH, frame)
    w = ar.philox_v(int(genv) & ar.M32, c1, c2, np.arange(npx, dtype=np.uint64), seed)
    return ar.u01_v(w[:, :3])


def latency_draw(genv, frame, seed, lo, hi):
    """The delay a fill draws: lo + min((int)(u * (hi - lo + 1)), hi - lo) with the product rounded to float32."""
    c1, c2 = ar.step_key(RNG_DEPTH, frame)
    u = ar.u01(ar.philox(int(genv) & ar.M32, c1, c2, LATENCY_PIXEL, seed)[0])
    return lo + min(int(F32(u * F32(hi - lo + 1))), hi - lo)


def masks(z, p, u2):
    """(far, edge, drop) of one float32 image [H, W]; edge and drop exclude far pixels, a pixel may be in both."""
    z = np.asarray(z, F32)
    far = z >= p.far
    edge = np.zeros(z.shape, bool)
    if p.edge_thresh > 0:
        for a, b, ea, eb in ((z[:, 1:], z[:, :-1], edge[:, 1:], edge[:, :-1]),
                             (z[1:, :], z[:-1, :], edge[1:, :], edge[:-1, :])):
            step = np.abs(a - b) > p.edge_thresh * np.minimum(a, b)  # float32 throughout; symmetric in (a, b)
            ea |= step
            eb |= step
    drop = np.asarray(u2, F32).reshape(z.shape) < p.dropout_p
    return far, edge & ~far, drop & ~far


def noisy(z, p, u, dtype=np.float64):
    """Before quantisation and clamping: (z + sigma n, n, rad, sigma) with n = rad cos(2 pi u1) (aux_ref.box_muller's
    even member) and sigma = noise_a + noise_b z^2, every array of z's shape."""
    z = np.asarray(z, F32)
    u = np.asarray(u, F32).reshape(z.shape + (3,))
    n, rad = ar.box_muller(u[..., 0], u[..., 1], False)
    if dtype == np.float64:
        z64 = z.astype(np.float64)
        sigma = np.float64(p.noise_a) + np.float64(p.noise_b) * z64 * z64
        return z64 + sigma * n, n, rad, sigma
    sigma = p.noise_a + p.noise_b * z * z  # float32, left to right: three roundings
    return z + sigma * n.astype(F32), n, rad, sigma.astype(np.float64)


def finish(zn, p, dtype=np.float64):
    """Quantise (when quant > 0) and clamp to [near, far]."""
    zn = np.asarray(zn, dtype)
    if p.quant > 0:
        zn = np.rint(zn / dtype(p.quant)) * dtype(p.quant)
    return np.minimum(np.maximum(zn, dtype(p.near)), dtype(p.far))


def sense(z, p, u, dtype=np.float64):
    """The sensed image v of one exact image z [H, W] from its uniforms [H, W, 3] (or [H W, 3])."""
    far, edge, drop = masks(z, p, np.asarray(u, F32).reshape(np.shape(z) + (3,))[..., 2])
    v = finish(noisy(z, p, u, dtype)[0], p, dtype)
    v = np.where(edge | drop, dtype(p.invalid_value), v)
    return np.where(far, dtype(p.far), v).astype(dtype)


def value_bar(z, n, rad, sigma):
    """The bar on |v - v_ref| of a kept pixel, noise on and quantisation off: sigma times aux_ref's bound on this
    Box-Muller followed by z + sigma n (mu = z, sd = sigma), plus 4 x 2^-24 sigma |n| for the three roundings of
    noise_a + noise_b z z.  The clamp to [near, far] does not widen it."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sigma > 0, np.asarray(z, np.float64) / sigma, 0.0)
    return sigma * ar.policy_noise_bound(rad, n, ratio) + 4.0 * 2.0 ** -24 * sigma * np.abs(n)


def state(n, p, fill=-7.0, dtype=np.float64):
    """The arrays a call works on, as a caller would allocate them (``fill``: what they hold before the first call)."""
    D = p.latency_max + 1
    return dict(ring=np.full((n, D, p.height, p.width), fill, dtype), head=np.full(n, int(fill), np.int32),
                latency=np.full(n, int(fill), np.int32), sensed=np.full((n, p.height, p.width), fill, dtype))


def advance(st, p, mode, flags, v, delays):
    """The ring's bookkeeping of one call on every env b: ``v[b]`` the frame's sensed image, ``delays[b]`` the delay a
    fill of env b would draw.  PUSH: a flagged env fills; RESET_ONLY: only flagged envs, filling; FILL: every env."""
    D = p.latency_max + 1
    for b in range(len(st["head"])):
        flagged = bool(flags[b])
        if mode == RESET_ONLY and not flagged:
            continue
        if mode != PUSH or flagged:
            st["latency"][b], st["head"][b] = delays[b], 0
            st["ring"][b, :] = v[b]
            st["sensed"][b] = v[b]
        else:
            h = (int(st["head"][b]) + 1) % D
            st["head"][b] = h
            st["ring"][b, h] = v[b]
            st["sensed"][b] = st["ring"][b, (h - int(st["latency"][b]) + D) % D]
    return st


def call(st, p, first_genv, seed, mode, flags, frame, depth, uniforms=None, dtype=np.float64):
    """lrl_sim_depth_sense on envs whose global ids start at ``first_genv``: depth [n, H, W] float32, flags [n],
    uniforms None or [n, H, W, 3].  Returns the per-env sensed images of this frame (before the ring) as well."""
    n, npx = len(depth), p.width * p.height
    u = [pixel_uniforms(first_genv + b, frame, seed, npx) if uniforms is None else uniforms[b] for b in range(n)]
    v = np.stack([sense(depth[b], p, u[b], dtype) for b in range(n)])
    delays = [latency_draw(first_genv + b, frame, seed, p.latency_min, p.latency_max) for b in range(n)]
    advance(st, p, mode, flags, v, delays)
    return v


def scene(n, height, width, far=3.0):
    """Synthetic exact images [n, H, W] float32: per env two tilted planes with a step between them along a slanted
    line, and a corner patch at ``far``.  Values stay inside (near, far) off the patch."""
    i, j = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    out = np.empty((n, height, width), F32)
    for b in range(n):
        near_plane = 0.6 + 0.05 * b + 0.004 * i + 0.002 * j
        far_plane = 1.7 + 0.1 * b + 0.006 * i - 0.003 * j
        z = np.where(j + 0.3 * i < 0.45 * width + b, near_plane, far_plane)
        z = np.where((i < 0.25 * height) & (j > 0.7 * width), far, z)
        out[b] = z.astype(F32)
    return out
