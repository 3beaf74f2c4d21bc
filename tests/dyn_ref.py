"""Rigid-body dynamics of the legged robot from forward kinematics and the mass tables alone, in numpy float64: the
independent reference the env step kernel's (and the CPU oracle's) physics is held to.

Nothing here imports the product or the oracle, and nothing restates their formulation (no spatial algebra, no mass
matrix, no recursive Newton-Euler).  The only ingredients are ``aux_ref.fk_mat`` (a chain of homogeneous transforms
and the textbook velocity recursion, itself pinned by tests/test_aux_ref.py), the table's masses, centres of mass and
inertias, and three facts of elementary mechanics about a system of rigid bodies:

    d/dt p            = sum of external forces                                   (total linear momentum)
    d/dt L_o + v_o x p = sum of external torques about o                         (angular momentum about a moving point o)
    axis . (d/dt L_sub,o + v_o x p_sub) = tau + axis . (external torque on the subtree about o)

the last one for the bodies distal to a revolute joint, o on the joint's axis: the only torque the rest of the robot
transmits about that axis is the actuator's.  Every momentum is read off the FK velocities (m v_c, (c - o) x m v_c +
R I R^T w), so it is linear in the velocity coordinates; its time derivative is the velocity-Jacobian times the
acceleration plus the change along the motion at fixed coordinates, taken as a central difference.

State x = (base origin o [3], base rotation R [3, 3] base-to-world, joint angles q [12]).  Velocity coordinates
nu [18] = (R^T W, R^T V, qd): the base's angular velocity and the velocity of the base body's centre of mass, both in
base axes, and the joint rates - the components a body-frame integrator advances.  ``nud`` is their componentwise time
derivative.  Rows of the 18 equations: 0-2 linear momentum (N), 3-5 angular momentum about the base origin (N m),
6-17 the joints (N m), in world axes.
"""
import numpy as np

import aux_ref as ar

EPS = 1e-6  # step of the central difference along the motion (s)
GROUPS = {"linear": slice(0, 3), "angular": slice(3, 6), "joint": slice(6, 18)}


def _sym(i6):
    """3 x 3 inertia of the table's six entries (xx, yy, zz, xy, xz, yz)."""
    xx, yy, zz, xy, xz, yz = (float(v) for v in i6)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def robot(table, payload=0.0, com=(0.0, 0.0, 0.0)):
    """The 13 dynamic bodies of a robot table (aux_ref's FK keys plus base_mass, base_inertia, link_mass, link_com,
    link_inertia): the base carries the payload (mass base_mass + payload, inertia scaled by the same ratio, centre
    of mass at the displacement ``com``), then hip, thigh and calf of every leg as tabulated (the calf row holds the
    fixed foot)."""
    mb = float(table["base_mass"])
    m, c, I, idx = [mb + float(payload)], [np.asarray(com, np.float64)], \
        [_sym(table["base_inertia"]) * ((mb + float(payload)) / mb)], [None]
    where = {(leg, link): b for b, (leg, link) in enumerate(zip(table["body_leg"], table["body_link"]))}
    idx[0] = list(table["body_leg"]).index(-1)
    for leg in range(4):
        for j in range(3):
            m.append(float(table["link_mass"][leg][j]))
            c.append(np.asarray(table["link_com"][leg][j], np.float64))
            I.append(_sym(table["link_inertia"][leg][j]))
            idx.append(where[leg, j])
    ax = np.asarray(table["joint_axis"], np.float64).reshape(12, 3)
    return dict(table=table, com=np.asarray(com, np.float64), mass=np.array(m), c=np.stack(c), I=np.stack(I),
                idx=np.array(idx), axis=ax / np.linalg.norm(ax, axis=1, keepdims=True))


def bodies(rb, x, nu):
    """Per dynamic body from FK: centre of mass c [13, 3], its velocity vc [13, 3], the angular velocity w [13, 3],
    R I R^T w [13, 3], R I R^T [13, 3, 3]; and the body origins o [13, 3] with their velocities vo [13, 3], the world
    joint axes [12, 3]."""
    o, R, q = x
    nu = np.asarray(nu, np.float64)
    pos, rot, vel, ang = ar.fk_mat(rb["table"], o, R, R @ nu[3:6], R @ nu[0:3], rb["com"], q, nu[6:18])
    pos, rot, vel, ang = (a[rb["idx"]] for a in (pos, rot, vel, ang))
    r = np.einsum("bij,bj->bi", rot, rb["c"])
    Iw = np.einsum("bij,bjk,blk->bil", rot, rb["I"], rot)
    return dict(c=pos + r, vc=vel + _cross(ang, r), w=ang, Iw=np.einsum("bij,bj->bi", Iw, ang), I=Iw, o=pos, vo=vel,
                axis=np.einsum("bij,bj->bi", rot[1:], rb["axis"]))


def _subtree(j):
    """Dynamic bodies distal to joint j (0..11): the links j % 3 .. 2 of leg j // 3."""
    return np.arange(1 + j, 1 + 3 * (j // 3) + 3)


SUB = np.zeros((12, 13))  # SUB[j, b] = 1: body b is distal to joint j
for _j in range(12):
    SUB[_j, _subtree(_j)] = 1.0


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _momenta(rb, x, nu):
    k = bodies(rb, x, nu)
    mv = rb["mass"][:, None] * k["vc"]
    p = mv.sum(0)
    L = (_cross(k["c"] - k["o"][0], mv) + k["Iw"]).sum(0)
    # per joint: sum over its subtree of (c - o_j) x m v_c + I w, the bodies taken relative to the base origin first
    psub = SUB @ mv
    Lsub = SUB @ (_cross(k["c"] - k["o"][0], mv) + k["Iw"]) - _cross(k["o"][1:] - k["o"][0], psub)
    return p, L, Lsub, psub, k


def momenta(rb, x, nu):
    """(total linear momentum [3], total angular momentum about the base origin [3], per joint the distal subtree's
    angular momentum about the joint origin [12, 3]), world axes.  All linear in ``nu``."""
    return _momenta(rb, x, nu)[:3]


def flow(x, nu, com, eps):
    """The configuration moved for the time ``eps`` at the velocity ``nu``: origin + eps v_origin, exp(eps [W]) R,
    q + eps qd (the origin moves at V - W x R com)."""
    o, R, q = x
    nu = np.asarray(nu, np.float64)
    W, V = R @ nu[0:3], R @ nu[3:6]
    return (np.asarray(o, np.float64) + eps * (V - _cross(W, R @ np.asarray(com, np.float64))),
            ar.rot_exp(eps * W) @ R, np.asarray(q, np.float64) + eps * nu[6:18])


def _centre(x):
    """The same configuration with the base origin at 0 (the dynamics are translation invariant; a long lever on
    rounded velocities otherwise enters the angular rows)."""
    return (np.zeros(3), np.asarray(x[1], np.float64), np.asarray(x[2], np.float64))


def _linear(rb, x, nud):
    """The part of the 18 left sides that is linear in the acceleration: (p, L, axis . Lsub) evaluated at the
    velocity coordinates ``nud`` (the momenta are linear in nu, so this is their velocity-Jacobian times nud)."""
    p, L, Lsub, _, k = _momenta(rb, x, np.asarray(nud, np.float64))
    return np.concatenate([p, L, np.einsum("ji,ji->j", k["axis"], Lsub)])


def drift(rb, x, nu, tau, g):
    """The 18 equations at zero acceleration, left side minus right side: the change of the momenta along the motion
    at fixed velocity coordinates (central difference over ``flow``), the transport terms of the moving reference
    points, minus gravity and ``tau``.  Evaluated with the base origin at 0."""
    x, g, tau = _centre(x), np.asarray(g, np.float64), np.asarray(tau, np.float64)
    p, _, _, psub, k = _momenta(rb, x, nu)
    fwd = _momenta(rb, flow(x, nu, rb["com"], EPS), nu)
    bwd = _momenta(rb, flow(x, nu, rb["com"], -EPS), nu)
    dp, dL, dLsub = ((fwd[i] - bwd[i]) / (2 * EPS) for i in range(3))
    mg = rb["mass"][:, None] * g[None, :]
    out = np.empty(18)
    out[0:3] = dp - mg.sum(0)
    out[3:6] = dL + _cross(k["vo"][0], p) - _cross(k["c"] - k["o"][0], mg).sum(0)
    for j in range(12):
        s = _subtree(j)
        oj, vj = k["o"][1 + j], k["vo"][1 + j]
        torque = _cross(k["c"][s] - oj, mg[s]).sum(0)
        out[6 + j] = k["axis"][j] @ (dLsub[j] + _cross(vj, psub[j]) - torque) - tau[j]
    return out


def residual(rb, x, nu, nud, tau, g, at_rest=None):
    """The 18 equations with the acceleration ``nud`` plugged in, left side minus right side: what external force
    (rows 0-2, N), external torque about the base origin (3-5, N m) and unaccounted joint torque (6-17, N m) the
    motion would need beyond gravity and ``tau``.  ``at_rest``: a ``drift`` of the same (x, nu, tau, g) computed
    before, when several accelerations are judged at one state."""
    return (drift(rb, x, nu, tau, g) if at_rest is None else at_rest) + _linear(rb, _centre(x), nud)


def jacobian(rb, x):
    """d residual / d nud [18, 18]: the momenta's velocity-Jacobian (the joint rows projected on their axes)."""
    return np.stack([_linear(rb, _centre(x), e) for e in np.eye(18)], 1)


def accel(rb, x, nu, tau, g):
    """The 18 generalised accelerations: the equations are affine in nud, residual = jacobian nud + drift."""
    return np.linalg.solve(jacobian(rb, x), -drift(rb, x, nu, tau, g))


def linear_momentum_rate(rb, x, nu, nud):
    """d/dt of the total linear momentum [3] (N): the sum of every external force, gravity included.  (The linear rows
    of ``residual`` are this minus m g.)"""
    x = _centre(x)
    fwd, bwd = (_momenta(rb, flow(x, nu, rb["com"], e), nu)[0] for e in (EPS, -EPS))
    return (fwd - bwd) / (2 * EPS) + _linear(rb, x, nud)[0:3]


def energy(rb, x, nu, g):
    """Kinetic plus potential energy from the FK velocities and positions: sum 1/2 m |v_c|^2 + 1/2 w . R I R^T w -
    m g . c."""
    k = bodies(rb, x, nu)
    return float(0.5 * (rb["mass"] * (k["vc"] ** 2).sum(1)).sum() + 0.5 * (k["w"] * k["Iw"]).sum()
                 - (rb["mass"] * (k["c"] @ np.asarray(g, np.float64))).sum())
