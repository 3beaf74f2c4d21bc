"""Numpy restatement of the headless camera (include/lrl.h: lrl_sim_render), the checker of tests/test_render_gpu.py.

It follows the header's definitions, not the kernel's code: classic quadratic ray / sphere and ray / capsule forms,
slabs in the box frame, brute force over the ground's triangles (no grid walk), no slack on triangle edges.
tests/test_render_ref.py pins it on scenes with analytic answers, so kernel-vs-checker is not circular.

    prims  = {"box": None | (centre[3], R[3, 3] world-from-box, half[3]),
              "spheres": [(s, centre[3], radius)], "capsules": [(c, a[3], b[3], radius)]}
    ground = None | ("plane",) | ("tris", T[n, 3, 3])            (z = 0, or world-frame triangles)
    camera = {"pos", "target" (world), "hfov_deg", "far", "width", "height"}
    trace(...) -> {"rgba" u8 [H, W, 4], "depth" [H, W], "ids" i32 [H, W], "cell" i8 [H, W]}

"cell" is 1 + the checkerboard parity on ground pixels and 0 elsewhere (the ids do not tell the two ground colours
apart; the colour checks use it to leave checkerboard edges out).
"""
import numpy as np

from lrl import _abi

MAX_SPHERES = _abi.MAX_SPHERES
ID_GROUND, ID_BOX, ID_SPHERE0, ID_CAPSULE0 = 1, 2, 3, 3 + _abi.MAX_SPHERES
SHADOW = _abi.RENDER_ID_SHADOW


def _c(v):  # a header constant as the kernel holds it: rounded to float32
    return np.asarray(v, np.float32).astype(np.float64)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def camera_basis(pos, target, dtype=np.float64):
    pos, target = np.asarray(pos, dtype), np.asarray(target, dtype)
    f = _unit(target - pos)
    r = np.cross(f, np.array([0, 0, 1], dtype))
    if np.sqrt(_dot(r, r)) < 1e-6:
        r = np.cross(f, np.array([0, 1, 0], dtype))
    r = _unit(r)
    return f, r, np.cross(r, f)


def camera_rays(camera, dtype=np.float64):
    """Unit ray directions [H * W, 3] (row-major pixels, row 0 at the top)."""
    W, H = int(camera["width"]), int(camera["height"])
    f, r, up = camera_basis(camera["pos"], camera["target"], dtype)
    th = np.tan(np.asarray(camera["hfov_deg"], dtype) * dtype(np.pi / 180) * dtype(0.5)).astype(dtype)
    j = np.arange(W, dtype=dtype)
    i = np.arange(H, dtype=dtype)
    u = (2 * (j + dtype(0.5)) / dtype(W) - 1) * th
    v = (1 - 2 * (i + dtype(0.5)) / dtype(H)) * th * dtype(H) / dtype(W)
    d = f[None, None] + u[None, :, None] * r[None, None] + v[:, None, None] * up[None, None]
    return _unit(d.reshape(-1, 3)).astype(dtype)


def _sphere(O, D, c, r):
    oc = O - c
    b = _dot(oc, D)
    disc = b * b - (_dot(oc, oc) - r * r)
    t = -b - np.sqrt(np.maximum(disc, 0))
    return np.where((disc > 0) & (t > 0), t, np.inf)


def _capsule(O, D, a, b, r):
    """Union of the cylinder side over the segment and the two end spheres; entry distance or inf."""
    t = np.minimum(_sphere(O, D, a, r), _sphere(O, D, b, r))
    ba = b - a
    baba = _dot(ba, ba)
    if baba > 0:
        oa = O - a
        bard, baoa, rdoa, oaoa = _dot(D, ba), _dot(oa, ba), _dot(D, oa), _dot(oa, oa)
        A = baba - bard * bard
        B = baba * rdoa - baoa * bard
        Cq = baba * oaoa - baoa * baoa - r * r * baba
        h = B * B - A * Cq
        ok = (A > 1e-12 * baba) & (h > 0)
        tc = (-B - np.sqrt(np.maximum(h, 0))) / np.where(ok, A, 1)
        y = baoa + tc * bard
        t = np.minimum(t, np.where(ok & (tc > 0) & (y >= 0) & (y <= baba), tc, np.inf))
    return t


def _box(O, D, c, R, h):
    """Slabs in the box frame; returns (t, outward normal of the entry face)."""
    ol = (O - c) @ R
    dl = D @ R
    par = np.abs(dl) < 1e-12
    inv = 1 / np.where(par, 1, dl)
    ta, tb = (-h - ol) * inv, (h - ol) * inv
    tn = np.where(par, -np.inf, np.minimum(ta, tb))
    tf = np.where(par, np.inf, np.maximum(ta, tb))
    miss = np.any(par & (np.abs(ol) > h), axis=-1)
    ax = np.argmax(tn, axis=-1)
    t0, t1 = np.max(tn, axis=-1), np.min(tf, axis=-1)
    t = np.where(~miss & (t0 <= t1) & (t0 > 0), t0, np.inf)
    sgn = -np.sign(np.take_along_axis(dl, ax[:, None], 1)[:, 0])
    return t, sgn[:, None] * R.T[ax]


def _tris(O, D, T, chunk=512):
    """Möller–Trumbore, two-sided, brute force: nearest t and its triangle's normal (not normalised)."""
    P = D.shape[0]
    best = np.full(P, np.inf, D.dtype)
    nrm = np.zeros((P, 3), D.dtype)
    for k in range(0, len(T), chunk):
        a = T[k:k + chunk, 0][None]
        e1, e2 = T[k:k + chunk, 1][None] - a, T[k:k + chunk, 2][None] - a
        pv = np.cross(D[:, None], e2)
        det = _dot(e1, pv)
        ok = np.abs(det) > 0
        inv = 1 / np.where(ok, det, 1)
        tv = O[:, None] - a
        u = _dot(tv, pv) * inv
        qv = np.cross(tv, e1)
        v = _dot(D[:, None], qv) * inv
        t = _dot(e2, qv) * inv
        t = np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t, np.inf)
        j = np.argmin(t, axis=1)
        tj = t[np.arange(P), j]
        better = tj < best
        best = np.where(better, tj, best)
        nrm = np.where(better[:, None], np.cross(e1[0], e2[0])[j], nrm)
    return best, nrm


def _in_view(T, camera):
    """The camera-relative triangles that can show in the image: a triangle with a vertex behind the camera plane is
    kept; otherwise the box of its vertices' image coordinates must meet the image (grown by a tenth); and its nearest
    vertex lies within far + its longest edge."""
    f, r, up = camera_basis(np.zeros(3), np.asarray(camera["target"], np.float64) - np.asarray(camera["pos"], np.float64))
    th = np.tan(np.deg2rad(float(camera["hfov_deg"])) / 2)
    tv = th * int(camera["height"]) / int(camera["width"])
    z = T @ f
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = (T @ r) / z, (T @ up) / z
    front = np.all(z > 1e-6, axis=1)
    lim_u, lim_v = 1.1 * th, 1.1 * tv
    seen = (u.min(1) <= lim_u) & (u.max(1) >= -lim_u) & (v.min(1) <= lim_v) & (v.max(1) >= -lim_v)
    edge = np.sqrt(np.max(np.sum((T - T[:, [1, 2, 0]]) ** 2, axis=2), axis=1))
    near = np.sqrt(np.min(np.sum(T * T, axis=2), axis=1)) <= float(camera["far"]) + edge  # rays end at far
    return T[(~front | seen) & near]


def _robot(prims, O, D, dtype):
    """Nearest robot primitive: (t, id, normal)."""
    P = D.shape[0]
    t = np.full(P, np.inf, dtype)
    ident = np.zeros(P, np.int32)
    n = np.zeros((P, 3), dtype)
    if prims.get("box") is not None:
        c, R, h = (np.asarray(x, dtype) for x in prims["box"])
        tb, nb = _box(O, D, c, R, h)
        m = tb < t
        t, ident, n = np.where(m, tb, t), np.where(m, ID_BOX, ident), np.where(m[:, None], nb, n)
    for s, c, r in prims.get("spheres", ()):
        c, r = np.asarray(c, dtype), dtype(r)
        ts = _sphere(O, D, c, r)
        m = ts < t
        with np.errstate(invalid="ignore"):
            ns = _unit(O + np.where(m, ts, 0)[:, None] * D - c)
        t, ident, n = np.where(m, ts, t), np.where(m, ID_SPHERE0 + s, ident), np.where(m[:, None], ns, n)
    for k, a, b, r in prims.get("capsules", ()):
        a, b, r = np.asarray(a, dtype), np.asarray(b, dtype), dtype(r)
        tc = _capsule(O, D, a, b, r)
        m = tc < t
        p = O + np.where(m, tc, 0)[:, None] * D
        ba = b - a
        L2 = _dot(ba, ba)
        y = np.clip(_dot(p - a, ba) / L2, 0, 1) if L2 > 0 else np.zeros(P, dtype)
        with np.errstate(invalid="ignore"):
            nc = _unit(p - a - y[:, None] * ba)
        t, ident, n = np.where(m, tc, t), np.where(m, ID_CAPSULE0 + k, ident), np.where(m[:, None], nc, n)
    return t, ident, n


def trace(prims, ground, camera, dtype=np.float64):
    dtype = np.dtype(dtype).type
    W, H = int(camera["width"]), int(camera["height"])
    far = dtype(camera["far"])
    o = np.asarray(camera["pos"], np.float64)
    D = camera_rays(camera, dtype)
    P = D.shape[0]
    # everything relative to the camera position (taken in float64: differences of nearby fp32 coordinates are exact)
    rel = {"box": None, "spheres": [], "capsules": []}
    if prims.get("box") is not None:
        c, R, h = prims["box"]
        rel["box"] = (np.asarray(c, np.float64) - o, R, h)
    rel["spheres"] = [(s, np.asarray(c, np.float64) - o, r) for s, c, r in prims.get("spheres", ())]
    rel["capsules"] = [(k, np.asarray(a, np.float64) - o, np.asarray(b, np.float64) - o, r)
                       for k, a, b, r in prims.get("capsules", ())]
    O = np.zeros((P, 3), dtype)
    t, ident, n = _robot(rel, O, D, dtype)
    keep = t < far
    t, ident = np.where(keep, t, np.inf), np.where(keep, ident, 0)
    if ground is not None:
        if ground[0] == "plane":
            oz = dtype(o[2])
            with np.errstate(divide="ignore", invalid="ignore"):
                tg = np.where((D[:, 2] < 0) & (oz > 0), -oz / D[:, 2], np.inf)
            ng = np.tile(np.array([0, 0, 1], dtype), (P, 1))
        else:
            T = _in_view(np.asarray(ground[1], np.float64) - o, camera).astype(dtype)
            tg, ng = _tris(O, D, T)
            with np.errstate(invalid="ignore", divide="ignore"):
                ng = _unit(ng)
            ng = np.where((_dot(ng, D) > 0)[:, None], -ng, ng)
        m = (tg < t) & (tg < far)
        t, ident, n = np.where(m, tg, t), np.where(m, ID_GROUND, ident), np.where(m[:, None], ng, n)
    hit = ident > 0
    tt = np.where(hit, t, 0)
    p = tt[:, None] * D
    light = _unit(_c(_abi.RENDER_LIGHT)).astype(dtype)
    amb = dtype(_c(_abi.RENDER_AMBIENT))
    ts, _, _ = _robot(rel, p + dtype(1e-3) * n, np.tile(light, (P, 1)), dtype)
    shadow = hit & np.isfinite(ts)
    parity = (np.floor(dtype(o[0]) + p[:, 0]).astype(np.int64) + np.floor(dtype(o[1]) + p[:, 1]).astype(np.int64)) & 1
    alb = np.tile(_c(_abi.RENDER_SKY), (P, 1))
    pal = {"ga": _c(_abi.RENDER_GROUND_A), "gb": _c(_abi.RENDER_GROUND_B), "base": _c(_abi.RENDER_BASE),
           "sph": _c(_abi.RENDER_SPHERE), "link": _c(_abi.RENDER_LINK)}
    g = ident == ID_GROUND
    alb[g & (parity == 0)] = pal["ga"]
    alb[g & (parity == 1)] = pal["gb"]
    alb[ident == ID_BOX] = pal["base"]
    alb[(ident >= ID_SPHERE0) & (ident < ID_CAPSULE0)] = pal["sph"]
    alb[ident >= ID_CAPSULE0] = pal["link"]
    k = amb + (1 - amb) * np.maximum(0, _dot(n, light)) * np.where(shadow, 0, 1)
    col = np.where(hit[:, None], alb * k[:, None], alb)
    rgb = np.floor(255 * np.clip(col, 0, 1) + 0.5).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((P, 1), 255, np.uint8)], 1).reshape(H, W, 4)
    ids = (ident | np.where(shadow, SHADOW, 0)).astype(np.int32).reshape(H, W)
    cell = np.where(g, 1 + parity, 0).astype(np.int8).reshape(H, W)
    return {"rgba": rgba, "depth": np.where(hit, t, np.inf).reshape(H, W), "ids": ids, "cell": cell}


def quat_to_matrix(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_from_state(rb, model):
    """The primitives lrl_sim_render draws, from one env's LRL_T_RIGID_BODY_STATE rows rb [B, 13] and the model tables
    model = {num_bodies, body_leg, body_link, num_spheres, sphere_body, sphere_pos, sphere_radius} (lrl_model's)."""
    rb = np.asarray(rb, np.float64)
    B, ns = int(model["num_bodies"]), int(model["num_spheres"])
    leg, link = np.asarray(model["body_leg"])[:B], np.asarray(model["body_link"])[:B]
    sb = np.asarray(model["sphere_body"])[:ns]
    sp = np.asarray(model["sphere_pos"], np.float32)[:ns]
    sr = np.asarray(model["sphere_radius"], np.float32)[:ns]
    pos = rb[:, 0:3]
    rot = [quat_to_matrix(rb[b, 3:7]) for b in range(B)]

    def body_of(l, k):
        for b in range(B):
            if leg[b] == l and link[b] == k:
                return b
        return -1

    def pose_body(s):  # a fixed foot's spheres are expressed in the calf frame
        b = sb[s]
        return body_of(leg[b], 2) if leg[b] >= 0 and link[b] > 2 else b

    def centre(s):
        b = pose_body(s)
        return pos[b] + rot[b] @ sp[s].astype(np.float64)

    prims = {"box": None, "spheres": [], "capsules": []}
    base = [s for s in range(ns) if leg[sb[s]] < 0]
    if base:  # the span of the base's shapes, in float32 as the library forms it
        lo = np.min(sp[base] - sr[base, None], axis=0)
        hi = np.max(sp[base] + sr[base, None], axis=0)
        c, h = np.float32(0.5) * (lo + hi), np.float32(0.5) * (hi - lo)
        if np.all(h > 0):
            prims["box"] = (pos[0] + rot[0] @ c.astype(np.float64), rot[0], h.astype(np.float64))
    for s in range(ns):
        if sr[s] > 0:
            prims["spheres"].append((s, centre(s), float(sr[s])))
    r = float(np.float32(_abi.RENDER_LINK_RADIUS))
    for l in range(_abi.NUM_LEGS):
        b = [body_of(l, k) for k in range(3)]
        for k in range(2):
            if b[k] >= 0 and b[k + 1] >= 0:
                prims["capsules"].append((3 * l + k, pos[b[k]], pos[b[k + 1]], r))
        best, far2 = -1, np.float32(-1)
        for s in range(ns):
            if leg[sb[s]] == l and link[sb[s]] >= 2 and sr[s] > 0:
                q = sp[s]
                d2 = np.float32(np.float32(q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
                if d2 > far2:
                    best, far2 = s, d2
        if b[2] >= 0 and best >= 0:
            prims["capsules"].append((3 * l + 2, pos[b[2]], centre(best), r))
    return prims


def grid_triangles(vtx, cam_pos, far):
    """The two triangles of every cell of the world-frame vertex grid vtx [rows, cols, 3] (lrl_sim_set_terrain's: (v(i,j),
    v(i+1,j+1), v(i,j+1)) and (v(i,j), v(i+1,j), v(i+1,j+1))) with a vertex within `far` of the camera in xy."""
    v = np.asarray(vtx, np.float64)
    a, b, c, d = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    T = np.concatenate([np.stack([a, d, b], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)])
    dist = np.sqrt(np.min(np.sum((T[:, :, :2] - np.asarray(cam_pos, np.float64)[:2]) ** 2, axis=2), axis=1))
    return T[dist <= far]


def boundary(ids, cell=None):
    """True where a pixel's id (and, when given, its checkerboard cell) differs from one of its 8 neighbours."""
    H, W = ids.shape
    out = np.zeros((H, W), bool)
    for img in ([ids] if cell is None else [ids, cell]):
        pad = np.pad(img, 1, mode="edge")
        for di in (0, 1, 2):
            for dj in (0, 1, 2):
                out |= pad[di:di + H, dj:dj + W] != img
    return out
