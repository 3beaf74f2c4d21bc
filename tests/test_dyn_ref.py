"""tests/dyn_ref.py pinned on mechanics it does not use, then the CPU oracle (oracle/lrl_oracle.c) held to it.

The reference builds its 18 equations from momenta and their rates.  Its pins come by other routes: free fall, the
power balance d/dt (T + V) = tau . qd with T and V straight from the FK velocities and positions, a compound pendulum
in closed form, and the constancy of the total momentum about a fixed world point under internal torques.

The oracle (float64 build) must then close all 18 equations in free flight within what the float32 rounding of its
wrapper's outputs can explain (``dyn_cases.output_rounding``: derived from the reference's own Jacobian, nothing taken
from the oracle), for both robots and for Go1 with random fixed joint rotations and axes; and in contact the rate of
its total linear momentum must be m g plus the contact forces it reports, on the plane under PGS and TGS and on a
rough mesh.  The float build's worst values on the GPU tests' input sets are printed: 4 x those are the kernel's bars
in tests/test_dyn_gpu.py.
"""
import copy

import numpy as np
import pytest

import aux_ref as ar
import dyn_cases as dc
import dyn_ref as dr
from helpers import robot_table
from oracle import oracle

G = np.array([0.0, 0.0, -9.81])


def _random_state(rng, M, spin=True):
    quat = rng.normal(size=4)
    x = (rng.uniform(-3, 3, 3), ar.quat_to_mat(quat), dc._joints(rng, M, 1)[0])
    nu = np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(-2, 2, 3), rng.uniform(-8, 8, 12)]) if spin else np.zeros(18)
    return x, nu


# =================================================================================================================
# the reference alone
# =================================================================================================================
@pytest.mark.parametrize("name", dc.MODELS)
def test_free_fall_from_rest(name):
    """At rest with no torque every body falls at g: nud = (0, R^T g, 0) at any pose, payload and displacement."""
    table, M, _ = robot_table(name)
    rng = np.random.default_rng(1)
    for _ in range(4):
        x, nu = _random_state(rng, M, spin=False)
        rb = dr.robot(table, rng.uniform(-1, 3), rng.uniform(-0.1, 0.1, 3))
        want = np.concatenate([np.zeros(3), x[1].T @ G, np.zeros(12)])
        # solve's error: cond(jacobian) ~ 1e4 (kg against kg m^2 of a calf) x 2^-53, on |g| ~ 10
        np.testing.assert_allclose(dr.accel(rb, x, nu, np.zeros(12), G), want, rtol=0, atol=1e-9)


def _moved(rb, x, nu, nud, h):
    return dr.flow(x, nu, rb["com"], h), nu + h * nud


@pytest.mark.parametrize("name", dc.MODELS)
def test_power_balance(name):
    """d/dt (T + V) = tau . qd along the reference's own acceleration, T and V from ``dyn_ref.energy`` (sums of
    1/2 m |v_c|^2, 1/2 w . I w and -m g . c over the FK bodies): a route that uses no momentum equation.  The
    derivative is a central difference over h = 1e-5 s of the state moved at (nu, nud): its truncation is h^2 / 6 of
    the energy's third derivative, ~ 1e-10 x the power scale |E| w^3 with w ~ 30 rad/s, and its rounding 2^-53 |E| /
    h ~ 1e-9; the bar is 1e-6 of sum |tau qd| + |E|."""
    table, M, _ = robot_table(name)
    rng = np.random.default_rng(2)
    h = 1e-5
    for _ in range(4):
        x, nu = _random_state(rng, M)
        rb = dr.robot(table, rng.uniform(-1, 3), rng.uniform(-0.1, 0.1, 3))
        tau = rng.uniform(-15, 15, 12)
        nud = dr.accel(rb, x, nu, tau, G)
        e1, e0 = dr.energy(rb, *_moved(rb, x, nu, nud, h), G), dr.energy(rb, *_moved(rb, x, nu, nud, -h), G)
        power = (e1 - e0) / (2 * h)
        scale = np.abs(tau * nu[6:]).sum() + abs(dr.energy(rb, x, nu, G))
        print(f"{name}: d/dt E {power:.6f} W, tau . qd {tau @ nu[6:]:.6f} W, scale {scale:.1f}")
        assert abs(power - tau @ nu[6:]) < 1e-6 * scale


def _calf_closed_form(table, rb, x, leg):
    """Of a calf turning about its fixed joint axis through the joint origin o, from the table and the calf's frame
    alone: (axis . I_o axis with I_o by the parallel-axis theorem, axis . ((c - o) x m g))."""
    b = [i for i, (l, k) in enumerate(zip(table["body_leg"], table["body_link"])) if (l, k) == (leg, 2)][0]
    Rc = ar.body_frames(table, x[0], x[1], x[2])[b, :3, :3]
    m, r, a = table["link_mass"][leg][2], table["link_com"][leg][2], rb["axis"][3 * leg + 2]
    Io = dr._sym(table["link_inertia"][leg][2]) + m * ((r @ r) * np.eye(3) - np.outer(r, r))
    return a @ Io @ a, (Rc @ a) @ np.cross(Rc @ r, m * G)


@pytest.mark.parametrize("name", ["mc", "go1_random_joints"])
def test_calf_is_a_compound_pendulum(name):
    """Everything proximal to a calf held still (base twist, its rate, the other joints' rates and accelerations all
    zero): the calf swings about a fixed axis, and its own equation closes at the compound pendulum's qdd = (tau +
    axis . ((c - o) x m g)) / (axis . I_o axis) at any spin.  (The six base rows then show the force that holds the
    base; they are not looked at.)  Nothing but float64 rounding and the central difference's 1e-9 is left."""
    table, M, _ = robot_table(name)
    rng = np.random.default_rng(3)
    for leg in range(4):
        x, _ = _random_state(rng, M, spin=False)
        rb = dr.robot(table, rng.uniform(-1, 3), rng.uniform(-0.1, 0.1, 3))
        j = 3 * leg + 2
        nu, nud, tau = np.zeros(18), np.zeros(18), np.zeros(12)
        nu[6 + j], tau[j] = rng.uniform(-8, 8), rng.uniform(-15, 15)
        inertia, gravity = _calf_closed_form(table, rb, x, leg)
        nud[6 + j] = (tau[j] + gravity) / inertia
        assert abs(gravity) > 1e-3 and abs(nud[6 + j]) > 10
        row = dr.residual(rb, x, nu, nud, tau, G)[6 + j]
        print(f"{name} leg {leg}: qdd {nud[6 + j]:.3f} rad/s^2 (gravity's share {gravity / inertia:.3f}), row {row:.3e} N m")
        assert abs(row) < 1e-8


@pytest.mark.parametrize("name", ["mc", "go1_random_joints"])
def test_calf_on_a_heavy_falling_robot(name):
    """The solve: with a 1e6 kg payload (the base then weighs and, scaled, resists turning 1e5 times what it did) and
    hip and thigh inertias of 1e6 kg m^2, nothing proximal to a calf turns, and the robot falls at g as one - in that
    falling frame the calf feels no weight, so qdd = tau / (axis . I_o axis).  What is left is the recoil of the
    proximal bodies, (the calf's inertia about o or its mass x a lever^2) over (theirs), ~ 1e-6 of qdd each: bar
    1e-5 |qdd|."""
    table, M, _ = robot_table(name)
    heavy = copy.deepcopy(table)
    heavy["link_inertia"][:, 0:2, 0:3] = 1e6
    rng = np.random.default_rng(3)
    for leg in range(4):
        x, _ = _random_state(rng, M, spin=False)
        rb = dr.robot(heavy, 1e6, rng.uniform(-0.1, 0.1, 3))
        j = 3 * leg + 2
        nu, tau = np.zeros(18), np.zeros(12)
        nu[6 + j], tau[j] = rng.uniform(-8, 8), rng.uniform(-15, 15)
        got = dr.accel(rb, x, nu, tau, G)
        want = tau[j] / _calf_closed_form(table, rb, x, leg)[0]
        print(f"{name} leg {leg}: qdd {got[6 + j]:.6f}, closed form {want:.6f}")
        assert abs(got[6 + j] - want) < 1e-5 * abs(want)
        np.testing.assert_allclose(got[3:6], x[1].T @ G, rtol=0, atol=1e-4)
        proximal = got[6:][np.arange(12) % 3 != 2]  # hips and thighs: |tau| / 1e6 kg m^2
        assert np.abs(proximal).max() < 1e-3


def _world_momenta(rb, x, nu):
    """Total linear momentum and angular momentum about the fixed world origin, straight from the FK bodies."""
    k = dr.bodies(rb, x, nu)
    mv = rb["mass"][:, None] * k["vc"]
    return mv.sum(0), (np.cross(k["c"], mv) + k["Iw"]).sum(0)


@pytest.mark.parametrize("name", dc.MODELS)
def test_internal_torques_leave_the_total_momentum_alone(name):
    """Without gravity the total momentum and the angular momentum about a fixed point of the world stay constant
    whatever the joint torques do (the accelerations differ by hundreds of rad/s^2 between the two torque sets).  The
    momenta here are taken about the world origin with the robot metres away from it - no moving reference point, no
    transport term - and differentiated along (nu, nud) by a central difference over h = 1e-5 s; bar 1e-6 of
    |p| (1 + |o|) / 1 s, six orders under the rates the torques cause in a single body."""
    table, M, _ = robot_table(name)
    rng = np.random.default_rng(4)
    h = 1e-5
    for _ in range(3):
        x, nu = _random_state(rng, M)
        rb = dr.robot(table, rng.uniform(-1, 3), rng.uniform(-0.1, 0.1, 3))
        acc = [dr.accel(rb, x, nu, tau, np.zeros(3)) for tau in (np.zeros(12), rng.uniform(-15, 15, 12))]
        assert np.abs(acc[0] - acc[1]).max() > 100
        for nud in acc:
            p1, L1 = _world_momenta(rb, *_moved(rb, x, nu, nud, h))
            p0, L0 = _world_momenta(rb, *_moved(rb, x, nu, nud, -h))
            scale = np.linalg.norm(_world_momenta(rb, x, nu)[0]) * (1 + np.linalg.norm(x[0])) + 1.0
            assert np.abs(p1 - p0).max() / (2 * h) < 1e-6 * scale, (p1 - p0) / (2 * h)
            assert np.abs(L1 - L0).max() / (2 * h) < 1e-6 * scale, (L1 - L0) / (2 * h)


@pytest.mark.parametrize("name", ["mc", "go1"])
def test_oracle_energy_is_the_references(name):
    """oracle.energy (the mass-matrix quadratic form plus m g z) equals the FK sum of the reference: both in float64
    from the same float32 inputs, a few thousand operations each, 1e-10 of |T| + |V|; and the oracle builds the base
    rotation from the float32 quaternion as it is, up to 2^-22 from the normalised one's (dyn_cases.output_rounding):
    that much of the base-frame velocities, twice that of T, and of every centre's height above the base origin."""
    table, M, P = robot_table(name)
    inp = dc.free_inputs(name, 37)
    g = np.array(P.gravity[:], np.float64)
    for e in range(0, 37, 4):
        rb = dr.robot(table, float(inp["payload"][e]), inp["com"][e].astype(np.float64))
        nu, R = dc.coordinates(inp["root"][e], inp["qd"][e])
        x = (inp["root"][e, 0:3].astype(np.float64), R, inp["q"][e].astype(np.float64))
        want = dr.energy(rb, x, nu, g)
        c = dr.bodies(rb, x, nu)["c"]
        pot = -(rb["mass"] * (c @ g)).sum()
        lever = (rb["mass"] * np.linalg.norm(c - x[0], axis=1)).sum() * np.linalg.norm(g)
        got = oracle.energy(M, P, inp["root"][e], inp["q"][e], inp["qd"][e], inp["payload"][e], inp["com"][e])
        bar = 1e-10 * (abs(want - pot) + abs(pot)) + 2.0 ** -22 * (2 * abs(want - pot) + lever)
        assert abs(got - want) < bar, (got, want, bar)


# =================================================================================================================
# the oracle against the reference
# =================================================================================================================
@pytest.mark.parametrize("name", dc.MODELS)
def test_oracle_free_flight_closes_every_equation(name):
    """One sub-step of the float64 oracle in free flight (self-collision off, no contact active): (nu+ - nu) / dt
    plugged into the reference's 18 equations leaves no more than its float32 outputs' rounding explains."""
    table, M, P = robot_table(name, **dc.FREE)
    inp = dc.free_inputs(name, 24)
    root1, qd1, con, cnt = dc.run_oracle(M, P, inp)
    assert (cnt == 0).all() and not con.any()
    res = dc.residuals(table, P, inp, {"oracle": (root1, qd1)})["oracle"]
    bar = np.stack([dc.output_rounding(table, P, inp, e, root1[e], qd1[e]) for e in range(24)])
    print(f"{name} free flight, float64 oracle: worst residual {dc.by_group(res)}, rounding bar {dc.by_group(bar)}, "
          f"worst residual / bar {np.max(np.abs(res) / bar):.3f}")
    assert (np.abs(res) <= bar).all(), np.argwhere(np.abs(res) > bar)[:8]


def _ground(name, ground, solver):
    """(table, M, P) of a contact case; the mesh is handed to both builds of the oracle."""
    if ground == "plane":
        return robot_table(name, **{"sim.physx.solver_type": solver})
    table, M, P = dc.rough_params(name)
    world, heights = dc.mesh(float(P.horizontal_scale), float(P.vertical_scale))[2:]
    oracle.set_terrain(world, heights)
    oracle.set_terrain(world, heights, library=oracle.cpu_lib())
    return table, M, P


CONTACT_CASES = [("plane", 1), ("plane", 0), ("mesh", 0)]  # (ground, solver_type: 1 TGS, 0 PGS; the mesh solves with PGS)


@pytest.mark.parametrize("ground,solver", CONTACT_CASES)
@pytest.mark.parametrize("name", ["mc", "go1"])
def test_oracle_contact_forces_balance_the_momentum(name, ground, solver):
    """Standing, tilted, low and penetrating robots: d/dt p - m g of the float64 oracle's sub-step equals the sum of
    the contact forces it reports, within the float32 rounding of its outputs (the linear rows of
    ``output_rounding`` plus half an ulp of every force component); on the plane every body's force points up and
    lies in the friction cone."""
    table, M, P = _ground(name, ground, solver)
    assert P.solver_tgs == int(solver == 1 and ground == "plane") and P.terrain_mesh == int(ground == "mesh")
    n = 32
    inp = dc.contact_inputs(name, n, ground)
    root1, qd1, con, cnt = dc.run_oracle(M, P, inp)
    for k in range(4):  # every kind of pose touches the ground
        assert (cnt[k::4] > 0).mean() >= 0.5, (dc.KINDS[k], cnt[k::4])
    res = dc.residuals(table, P, inp, {"oracle": (root1, qd1)}, tau=np.zeros((n, 12)))["oracle"][:, 0:3]
    f = con.astype(np.float64)
    err = np.abs(res - f.sum(1))
    bar = np.stack([dc.output_rounding(table, P, inp, e, root1[e], qd1[e])[0:3] for e in range(n)])
    bar += (np.spacing(np.abs(con)).astype(np.float64) / 2).sum(1)
    print(f"{name} {ground} solver {solver}: worst |d/dt p - m g - sum F| {err.max():.3e} N at forces up to "
          f"{np.abs(f).max():.0f} N, worst error / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), np.argwhere(err > bar)[:8]
    if ground == "plane":
        assert dc.cone_violation(P, inp, con).max() <= 0


# =================================================================================================================
# the float build on the GPU tests' inputs
# =================================================================================================================
def float_build_free(name, n):
    """Worst residual per row group of the float build (liblrl_cpu.so) on ``free_inputs(name, n)``."""
    table, M, P = robot_table(name, **dc.FREE)
    inp = dc.free_inputs(name, n)
    root1, qd1, _, cnt = dc.run_oracle(M, P, inp, library=oracle.cpu_lib())
    assert (cnt == 0).all()
    return dc.by_group(dc.residuals(table, P, inp, {"float": (root1, qd1)})["float"])


@pytest.mark.parametrize("n", [256, 37])
@pytest.mark.parametrize("name", ["mc", "go1"])
def test_float_build_free_flight(name, n):
    """The same source in float on the GPU test's free-flight inputs: its worst residuals (the kernel's bars are 4 x
    these) stay under 1e-5 of the largest single term of their equations - 2^-24 x a few hundred operations - so a
    1e-4 relative error of any term would show."""
    table, M, P = robot_table(name, **dc.FREE)
    worst = float_build_free(name, n)
    inp = dc.free_inputs(name, n)
    root1, qd1, _, _ = dc.run_oracle(M, P, inp)
    dt, scale = float(P.sim_dt), np.zeros(18)
    for e in range(0, n, 8):
        rb = dr.robot(table, float(inp["payload"][e]), inp["com"][e].astype(np.float64))
        nu, R = dc.coordinates(inp["root"][e], inp["qd"][e])
        nud = (dc.coordinates(root1[e], qd1[e])[0] - nu) / dt
        scale = np.maximum(scale, np.abs(dr.jacobian(rb, (np.zeros(3), R, inp["q"][e].astype(np.float64)))) @ np.abs(nud))
    print(f"{name} n={n} free flight, float build: worst residual {worst}; largest terms {dc.by_group(scale[None])}")
    for k, s in dr.GROUPS.items():
        assert 0 < worst[k] < 1e-5 * scale[s].max(), (k, worst[k], scale[s].max())


@pytest.mark.parametrize("ground,solver", CONTACT_CASES)
@pytest.mark.parametrize("n", [256, 37])
@pytest.mark.parametrize("name", ["mc", "go1"])
def test_float_build_contact_balance(name, n, ground, solver):
    """The float build's normalised balance error |d/dt p - m g - sum F| / (m |g| + sum |F| of the float64 oracle) on
    the GPU test's contact inputs (the kernel's bar is 4 x the worst): under 1e-5, and the cone holds on the plane."""
    table, M, P = _ground(name, ground, solver)
    inp = dc.contact_inputs(name, n, ground)
    ref = dc.run_oracle(M, P, inp)
    flt = dc.run_oracle(M, P, inp, library=oracle.cpu_lib())
    err = dc.balance_error(table, P, inp, {"float64": ref[:3], "float": flt[:3]}, ref[2])
    print(f"{name} n={n} {ground} solver {solver}: worst normalised balance error float64 {err['float64'].max():.3e}, "
          f"float {err['float'].max():.3e}; envs in contact {(ref[3] > 0).mean():.2f}")
    assert 0 < err["float"].max() < 1e-5
    if ground == "plane":
        assert dc.cone_violation(P, inp, flt[2]).max() <= 0
