"""Numpy restatement of the egocentric depth camera (include/lrl.h: lrl_sim_depth), the checker of
tests/test_depth_gpu.py.

It makes its own rays from (base position, base quaternion, camera) as the header defines them and reuses
tests/render_ref.py for the rest: the primitives of an env (scene_from_state), the ray / primitive forms (_robot: classic
quadratics, slabs in the box frame), brute force over the ground's triangles (_tris: no grid walk, no slack on edges).
tests/test_depth_ref.py pins it on scenes with analytic answers, so kernel-vs-checker is not circular.

    camera = {"pos" [3] (base frame), "pitch_deg", "hfov_deg", "near", "far", "width", "height"}
    prims  = render_ref's, or None (LRL_DEPTH_NO_ROBOT)
    ground = None | ("plane",) | ("tris", T[n, 3, 3])            (z = 0, or world-frame triangles)
    trace(...) -> {"depth" [H, W], "ids" i32 [H, W]}

With dtype=float32 the camera frame, the rays and every intersection are formed in float32 (in the checker's own order
of operations): the distance between that and the float64 run is the checker's measure of what fp32 costs.
"""
import numpy as np

import render_ref as rr

ID_GROUND = rr.ID_GROUND


def quat_matrix(q, dtype=np.float64):
    """World-from-base rotation of the xyzw quaternion, formed in dtype."""
    if np.dtype(dtype) == np.float64:
        return rr.quat_to_matrix(q)
    x, y, z, w = (dtype(v) for v in q)
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype)


def camera_frame(base_pos, base_quat, camera, dtype=np.float64):
    """(o, f, r, up) of the header: o = p + R pos, f = R (cos p, 0, -sin p), r = R (0, -1, 0), up = R (sin p, 0, cos p)."""
    dtype = np.dtype(dtype).type
    R = quat_matrix(base_quat, dtype)
    p = np.asarray(base_pos, dtype)
    pitch = dtype(camera["pitch_deg"]) * dtype(np.pi / 180)
    cp, sp = np.cos(pitch).astype(dtype), np.sin(pitch).astype(dtype)
    o = p + R @ np.asarray(camera["pos"], dtype)
    f = R @ np.array([cp, 0, -sp], dtype)
    r = R @ np.array([0, -1, 0], dtype)
    up = R @ np.array([sp, 0, cp], dtype)
    return o.astype(dtype), f.astype(dtype), r.astype(dtype), up.astype(dtype)


def pixel_uv(camera, dtype=np.float64, duv=(0.0, 0.0)):
    """lrl_camera's image coordinates (u [W], v [H]), shifted by duv."""
    dtype = np.dtype(dtype).type
    W, H = int(camera["width"]), int(camera["height"])
    th = np.tan(dtype(camera["hfov_deg"]) * dtype(np.pi / 180) * dtype(0.5)).astype(dtype)
    j, i = np.arange(W, dtype=dtype), np.arange(H, dtype=dtype)
    u = (2 * (j + dtype(0.5)) / dtype(W) - 1) * th + dtype(duv[0])
    v = (1 - 2 * (i + dtype(0.5)) / dtype(H)) * th * dtype(H) / dtype(W) + dtype(duv[1])
    return u.astype(dtype), v.astype(dtype)


def rays(camera, f, r, up, dtype=np.float64, duv=(0.0, 0.0)):
    """Unit directions [H * W, 3] (row-major, row 0 at the top) and 1 + u^2 + v^2 per pixel."""
    dtype = np.dtype(dtype).type
    u, v = pixel_uv(camera, dtype, duv)
    d = f[None, None] + u[None, :, None] * r[None, None] + v[:, None, None] * up[None, None]
    d = d.reshape(-1, 3)
    d = (d / np.sqrt(np.sum(d * d, axis=1))[:, None]).astype(dtype)
    s = (1 + u[None, :] ** 2 + v[:, None] ** 2).reshape(-1).astype(dtype)
    return d, s


def trace(prims, ground, base_pos, base_quat, camera, dtype=np.float64, duv=(0.0, 0.0)):
    dtype = np.dtype(dtype).type
    W, H = int(camera["width"]), int(camera["height"])
    near, far = dtype(np.float32(camera["near"])), dtype(np.float32(camera["far"]))
    o, f, r, up = camera_frame(base_pos, base_quat, camera, dtype)
    D, s = rays(camera, f, r, up, dtype, duv)
    P = D.shape[0]
    tmax = far * np.sqrt(s)  # planar distance `far` along each ray
    o64 = o.astype(np.float64)
    O = np.zeros((P, 3), dtype)
    t = np.full(P, np.inf, dtype)
    ident = np.zeros(P, np.int32)
    if prims is not None:
        # relative to the camera position (differences taken in float64: of nearby fp32 coordinates they are exact)
        rel = {"box": None, "spheres": [], "capsules": []}
        if prims.get("box") is not None:
            c, R, h = prims["box"]
            rel["box"] = (np.asarray(c, np.float64) - o64, R, h)
        rel["spheres"] = [(k, np.asarray(c, np.float64) - o64, rad) for k, c, rad in prims.get("spheres", ())]
        rel["capsules"] = [(k, np.asarray(a, np.float64) - o64, np.asarray(b, np.float64) - o64, rad)
                           for k, a, b, rad in prims.get("capsules", ())]
        t, ident, _ = rr._robot(rel, O, D, dtype)
        keep = t < tmax
        t, ident = np.where(keep, t, np.inf), np.where(keep, ident, 0)
    if ground is not None:
        if ground[0] == "plane":
            oz = dtype(o[2])
            with np.errstate(divide="ignore", invalid="ignore"):
                tg = np.where((D[:, 2] < 0) & (oz > 0), -oz / D[:, 2], np.inf)
        else:
            T = np.asarray(ground[1], np.float64) - o64
            T = T[np.any(T @ f.astype(np.float64) > 0, axis=1)]  # (a triangle wholly behind the camera plane is unseen)
            tg, _ = rr._tris(O, D, T.astype(dtype))
        m = (tg < t) & (tg < tmax)
        t, ident = np.where(m, tg, t), np.where(m, ID_GROUND, ident)
    hit = ident > 0
    z = np.where(hit, t, 0) * np.sum(D * f[None], axis=1)
    depth = np.where(hit, np.minimum(np.maximum(z, near), far), far)
    return {"depth": depth.reshape(H, W), "ids": ident.astype(np.int32).reshape(H, W)}


def quiet_ground(ground, base_pos, base_quat, camera, shift=1e-5, span=1e-3):
    """Ground pixels away from every depth discontinuity, from the float64 checker alone (ground-on-ground occlusion
    edges are in no id image): traced unperturbed and with (u, v) shifted by +-shift, the five depths of a quiet pixel
    are all ground and span at most `span` of the depth.  (A continuous facet moves <= shift / sin(grazing angle)
    relative: 6e-4 at one degree; an occlusion edge jumps by far more.)  Returns (unperturbed trace, quiet mask)."""
    runs = [trace(None, ground, base_pos, base_quat, camera, np.float64, duv)
            for duv in ((0, 0), (shift, 0), (-shift, 0), (0, shift), (0, -shift))]
    z = np.stack([r["depth"] for r in runs])
    allg = np.all(np.stack([r["ids"] for r in runs]) == ID_GROUND, axis=0)
    quiet = allg & (z.max(0) - z.min(0) <= span * z[0])
    return runs[0], quiet


def boundary(ids):
    return rr.boundary(ids)
