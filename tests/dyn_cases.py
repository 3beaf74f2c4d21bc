"""Input sets and evaluation shared by tests/test_dyn_ref.py (CPU: the oracle's two builds against tests/dyn_ref.py)
and tests/test_dyn_gpu.py (the env step kernel against it): states written as float32 exactly as every build
receives them, one physics sub-step each, judged through ``dyn_ref.residual``.

Free flight: the base 5 m up at any orientation, joints at least 0.3 rad inside their limits, |qd| <= 8, |tau| <= 15,
payload in [-1, 3], centre-of-mass displacement within 0.1 - no contact, limit or self-contact row can be active, so
(nu+ - nu) / dt is the model's unconstrained acceleration and every one of the 18 equations must close.

Contact: standing, tilted, low and penetrating poses on the plane or on a synthetic rough mesh (a slope plus ripples
plus steps), self-contact candidates more than 0.02 apart.  Whatever the solver did, the rate of the total linear
momentum minus m g is the sum of the external forces, which are the contact forces the step reports.
"""
import functools

import numpy as np

import aux_ref as ar
import dyn_ref as dr
from helpers import make_rough, robot_table
from oracle import oracle

F32 = np.float32
MODELS = ("mc", "go1", "go1_random_joints")
KINDS = ("standing", "tilted", "low", "penetrating")
FREE = {"asset.self_collisions": 1}  # Isaac Gym's filter semantics: 1 switches self-collision off
MESH_G, MESH_BORDER = 120, 2.0


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _joints(rng, M, n):
    lo, hi = np.array(M.dof_lower[:], np.float64), np.array(M.dof_upper[:], np.float64)
    return rng.uniform(lo + 0.3, hi - 0.3, (n, 12))


def _dr(rng, n):
    return dict(payload=rng.uniform(-1, 3, n).astype(F32), com=rng.uniform(-0.1, 0.1, (n, 3)).astype(F32),
                friction=rng.uniform(0.05, 4.5, n).astype(F32), restitution=rng.uniform(0, 1, n).astype(F32))


def torque_actions(P, tau):
    """Actions whose 'T'-control torque (action x action_scale, x hip_scale_reduction at the hips, motor strength 1)
    is ``tau``, and that torque as float32 arithmetic gives it back.  The hips' torques are scaled by 0.8 first: the
    action clip (100) caps them at 12.5."""
    tau = np.array(tau, np.float64)
    tau[:, 0::3] *= 0.8
    scale = np.full(12, P.action_scale, F32)
    act = (np.asarray(tau, np.float64) / scale / np.where(np.arange(12) % 3 == 0, P.hip_scale_reduction, 1.0)).astype(F32)
    t = act * scale
    t[:, 0::3] = t[:, 0::3] * F32(P.hip_scale_reduction)
    assert np.abs(act).max() < P.clip_actions and (np.abs(t) < np.array(P.torque_limits[:], F32)).all()
    return act, t.astype(F32)


@functools.lru_cache(None)
def free_inputs(name, n):
    _, M, P = robot_table(name, **FREE)
    rng = np.random.default_rng([MODELS.index(name), n, 1])
    quat = rng.normal(size=(n, 4))
    root = np.zeros((n, 13))
    root[:, 0:2], root[:, 2] = rng.uniform(-10, 10, (n, 2)), 5.0
    root[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    root[:, 7:10], root[:, 10:13] = rng.uniform(-2, 2, (n, 3)), rng.uniform(-5, 5, (n, 3))
    act, tau = torque_actions(P, rng.uniform(-15, 15, (n, 12)))
    return dict(root=root.astype(F32), q=_joints(rng, M, n).astype(F32), qd=rng.uniform(-8, 8, (n, 12)).astype(F32),
                act=act, tau=tau, **_dr(rng, n))


@functools.lru_cache(None)
def mesh(hs, vs):
    """The synthetic rough ground: a 0.15 slope along x, 3 cm ripples and 8 cm steps every 0.8 m along y, as a
    MESH_G x MESH_G grid of int16 samples (x vs) at spacing ``hs``.  (vertices [G, G, 3] float32 with x, y from 0 as
    lrl_sim_set_terrain takes them, samples, the same vertices in the world frame, heights in metres)."""
    i, j = np.meshgrid(np.arange(MESH_G), np.arange(MESH_G), indexing="ij")
    x, y = i * hs, j * hs
    h = 0.15 * x + 0.03 * np.sin(3.0 * x) * np.cos(2.5 * y) + 0.08 * np.floor(y / 0.8)
    samples = np.ascontiguousarray(np.round(h / vs).astype(np.int16))
    heights = samples.astype(F32) * F32(vs)
    vtx = np.stack([x, y, heights.astype(np.float64)], -1).astype(F32)
    world = vtx.copy()
    world[..., :2] -= F32(MESH_BORDER)
    return vtx, samples, world, heights


def rough_params(name, **over):
    """(table, lrl_model, params with terrain_mesh = 1) of ``name`` for the synthetic mesh."""
    table, M, _ = robot_table(name)
    P = make_rough("mc" if name == "mc" else "go1", border_size=MESH_BORDER, **over)[3]
    return table, M, P


@functools.lru_cache(None)
def contact_inputs(name, n, ground):
    """Env e is of kind KINDS[e % 4].  ``ground``: "plane" or "mesh"."""
    _, M, P = robot_table(name) if ground == "plane" else rough_params(name)
    rng = np.random.default_rng([MODELS.index(name), n, 2 + (ground == "mesh")])
    kind = np.arange(n) % 4
    h0 = float(P.base_init_state[2])
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(1.0, 7.0, (n, 2))
    z = np.choose(kind, [h0 + rng.uniform(-0.04, 0.0, n), h0 + rng.uniform(-0.04, 0.02, n), rng.uniform(0.08, 0.15, n),
                         h0 - rng.uniform(0.05, 0.10, n)])
    if ground == "mesh":
        hm = mesh(float(P.horizontal_scale), float(P.vertical_scale))[3]
        ci = ((root[:, 0:2] + MESH_BORDER) / P.horizontal_scale).astype(int)
        z += np.array([hm[i:i + 2, j:j + 2].mean() for i, j in ci])  # the ground under the base
    root[:, 2] = z
    ang = rng.normal(size=(n, 3)) * np.where(kind == 1, 0.5, 0.1)[:, None]
    ang[:, 2] = rng.uniform(-np.pi, np.pi, n)
    for e in range(n):
        root[e, 3:7] = _mat_quat(ar.rot_exp(np.array([0, 0, ang[e, 2]])) @ ar.rot_exp(np.array([ang[e, 0], ang[e, 1], 0])))
    root[:, 7:10], root[:, 10:13] = rng.normal(size=(n, 3)) * 0.3, rng.normal(size=(n, 3)) * 0.5
    lo, hi = np.array(M.dof_lower[:], np.float64), np.array(M.dof_upper[:], np.float64)
    q = np.empty((n, 12), F32)
    for e in range(n):
        while True:  # no self-contact candidate within 0.02 (contact_offset is 0.01)
            q[e] = np.clip(np.array(P.default_dof_pos[:]) + rng.normal(size=12) * 0.2, lo + 0.3, hi - 0.3)
            if oracle.self_pairs(M, q[e])[1].min() > 0.02:
                break
    act, tau = torque_actions(P, rng.uniform(-15, 15, (n, 12)))
    return dict(root=root.astype(F32), q=q, qd=rng.normal(size=(n, 12)).astype(F32), act=act, tau=tau, **_dr(rng, n))


def _mat_quat(R):
    """Quaternion (x, y, z, w) of a rotation matrix with trace > -1 (tilts far from a half turn)."""
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 4 * w * w]) / (4 * w)


# ---------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------
def run_oracle(M, P, inp, library=None, tau=None):
    """One cold-started sub-step of every env through the oracle (``library``: oracle.cpu_lib() for the float
    build): (root [n, 13], qd [n, 12], contact forces [n, B, 3], active ground contacts [n])."""
    n = inp["root"].shape[0]
    tau = inp["tau"] if tau is None else tau
    root, qd, con, cnt = (np.zeros((n, 13), F32), np.zeros((n, 12), F32), np.zeros((n, M.num_bodies, 3), F32),
                          np.zeros(n, np.int64))
    for e in range(n):
        root[e], _, qd[e], con[e], cnt[e] = oracle.physics_substep(
            M, P, inp["root"][e], inp["q"][e], inp["qd"][e], tau[e], inp["friction"][e], inp["restitution"][e],
            inp["payload"][e], inp["com"][e], library=library)
    assert (cnt >= 0).all()
    return root, qd, con, cnt


def coordinates(root, qd):
    """nu = (R^T W, R^T V, qd) of a root state row and joint rates (float32, widened), with R."""
    root = np.asarray(root, np.float64)
    R = ar.quat_to_mat(root[3:7])
    return np.concatenate([R.T @ root[10:13], R.T @ root[7:10], np.asarray(qd, np.float64)]), R


def residuals(table, P, inp, results, tau=None):
    """``dyn_ref.residual`` [n, 18] of each entry of ``results`` {label: (root after [n, 13], qd after [n, 12])}:
    the acceleration is (nu+ - nu) / sim_dt, nu+ read with the orientation after the step (the step converts its
    body-frame velocities with the new orientation).  tau = 0 rows 0-2 are d/dt p - m g."""
    n = inp["root"].shape[0]
    tau = np.asarray(inp["tau"] if tau is None else tau, np.float64)
    g, dt = np.array(P.gravity[:], np.float64), float(P.sim_dt)
    out = {k: np.empty((n, 18)) for k in results}
    for e in range(n):
        rb = dr.robot(table, float(inp["payload"][e]), inp["com"][e].astype(np.float64))
        nu, R = coordinates(inp["root"][e], inp["qd"][e])
        x = (inp["root"][e, 0:3].astype(np.float64), R, inp["q"][e].astype(np.float64))
        rest = dr.drift(rb, x, nu, tau[e], g)
        for k, (root1, qd1) in results.items():
            out[k][e] = dr.residual(rb, x, nu, (coordinates(root1[e], qd1[e])[0] - nu) / dt, tau[e], g, at_rest=rest)
    return out


def by_group(res):
    """Worst |residual| per row group (N, N m, N m)."""
    return {k: float(np.abs(res[:, s]).max()) for k, s in dr.GROUPS.items()}


def balance_error(table, P, inp, results, scale_forces):
    """Per env |d/dt p - m g - sum_b F_b| / (m |g| + sum_b |F_b| of ``scale_forces``) of each entry of ``results``
    {label: (root after, qd after, contact forces [n, B, 3])}: the normalised momentum balance, and the mass m g."""
    res = residuals(table, P, inp, {k: v[:2] for k, v in results.items()}, tau=np.zeros((inp["root"].shape[0], 12)))
    mass = float(table["base_mass"]) + inp["payload"].astype(np.float64) + float(np.sum(table["link_mass"]))
    norm = mass * np.linalg.norm(P.gravity[:]) + np.linalg.norm(scale_forces.astype(np.float64), axis=2).sum(1)
    return {k: np.linalg.norm(res[k][:, 0:3] - results[k][2].astype(np.float64).sum(1), axis=1) / norm for k in results}


def cone_violation(P, inp, forces):
    """Per env the worst over the bodies of -F_z and of |F_xy| - mu F_z less an allowance (plane ground; mu = (env +
    ground friction) / 2): positive where a body's force points down or leaves the cone.  The allowance is 16 x 2^-24
    x mu F_z + 2^-24 |F|: the projection's division and products, the sum over a body's spheres and the division by
    dt, each a float32 rounding or two."""
    f = forces.astype(np.float64)
    mu = 0.5 * (inp["friction"].astype(np.float64) + float(P.ground_friction))[:, None]
    t = np.linalg.norm(f[..., 0:2], axis=2)
    return np.maximum(-f[..., 2], t - mu * f[..., 2] * (1 + 2.0 ** -20) - 2.0 ** -24 * np.linalg.norm(f, axis=2)).max(1)


def output_rounding(table, P, inp, e, root1, qd1):
    """What float32 rounding at the step's interface can put into one env's 18 residuals.  The step returns W, V, the
    quaternion and qd rounded to float32: a component of nu+ = R+^T W+ moves by at most sum_k |R+_ki| ulp(W+_k) / 2
    plus |W+| times the angle 2^-23 the quaternion's rounding can turn R+ by (four components within 2^-25 each:
    |dq| <= 2^-24, a rotation by at most 2 |dq|); likewise V+; qd+ by ulp(qd+) / 2.  The inputs are float32 values
    taken exactly, but the input quaternion is a unit one rounded, |q| = 1 + e with |e| <= 2^-24: a step that builds
    its matrix without normalising reads R + 2 e (R - 1), up to 2^-22 |W| away in nu.  All divided by dt and pushed
    through |d residual / d nud| of the reference.

    The table's fixed joint quaternions and axes are float32 too, unit vectors rounded (exactly unit for both real
    robots: this term is then zero).  The reference normalises them; a step that does not reads a joint's rotation
    up to 4 |e_quat| + 2 |e_axis| away (|e| = | |.| - 1 |, the quaternion enters squared, the axis through a a^T and
    once more as the direction of the joint's rate).  Every term of a joint's row is a product along its leg's chain,
    every term of the base rows along all four: the row's terms, sum_i |d residual / d nud_i| |nud_i| + |the rest|
    + |tau|, times the sum of those deviations over the leg (all legs)."""
    rb = dr.robot(table, float(inp["payload"][e]), inp["com"][e].astype(np.float64))
    R = ar.quat_to_mat(inp["root"][e, 3:7].astype(np.float64))
    R1 = ar.quat_to_mat(root1[3:7].astype(np.float64))
    half_ulp = lambda a: np.spacing(np.abs(a).astype(F32)).astype(np.float64) / 2
    d = np.empty(18)
    for sl, rows in ((slice(0, 3), slice(10, 13)), (slice(3, 6), slice(7, 10))):
        d[sl] = (np.abs(R1).T @ half_ulp(root1[rows]) + 2.0 ** -23 * np.linalg.norm(root1[rows].astype(np.float64))
                 + 2.0 ** -22 * np.linalg.norm(inp["root"][e, rows].astype(np.float64)))
    d[6:18] = half_ulp(qd1)
    x = (np.zeros(3), R, inp["q"][e].astype(np.float64))
    A, dt = np.abs(dr.jacobian(rb, x)), float(P.sim_dt)
    off = lambda v: np.abs(np.linalg.norm(np.asarray(v, np.float64), axis=-1) - 1.0)
    leg = (4 * off(table["joint_quat"]) + 2 * off(table["joint_axis"])).sum(1)  # per leg
    if not leg.any():
        return A @ d / dt
    nu = coordinates(inp["root"][e], inp["qd"][e])[0]
    nud = (coordinates(root1, qd1)[0] - nu) / dt
    tau = inp["tau"][e].astype(np.float64)
    terms = A @ np.abs(nud) + np.abs(dr.drift(rb, x, nu, tau, np.array(P.gravity[:], np.float64)) + np.pad(tau, (6, 0)))
    terms[6:] += np.abs(tau)
    return A @ d / dt + terms * np.concatenate([np.full(6, leg.sum()), np.repeat(leg, 3)])
