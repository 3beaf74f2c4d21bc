"""Plain numpy references for the non-step env kernels (csrc/lrl_aux.hip, observe_kernel): the counter RNG, forward
kinematics of the robot table, and the small list / shift / mean operations; and for the draws the step and act
kernels take from the counter RNG themselves (observation noise, pushes, the per-step redraw, policy noise).  Nothing here imports the product; the
references work in float64 unless a ``dtype`` says otherwise, and tests/test_aux_ref.py pins them on facts from
outside this repository's kernels (Random123's known answers, finite differences, closed forms).
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (include/lrl_philox.h restated in Python integers)
# ---------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF
RNG_OBS_NOISE, RNG_DR, RNG_INIT, RNG_POLICY, RNG_RESET, RNG_PUSH, RNG_TERRAIN = 1, 2, 3, 4, 5, 6, 7


def philox(c0, c1, c2, c3, seed):
    """lrl_philox(c0, c1, c2, c3, seed): counter (c0..c3), key = the two 32-bit words of ``seed`` (low word first)."""
    c0, c1, c2, c3 = (int(c) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u01(x):
    """lrl_u01: the top 24 bits as a float32 in [0, 1)."""
    return np.float32(int(x) >> 8) * np.float32(2.0 ** -24)


def draw32(u, span, lo):
    """u * span + lo in float32 with both roundings (the kernels compile these lines uncontracted)."""
    return np.float32(np.float32(u) * np.float32(span)) + np.float32(lo)


def randomize_draws(genv, seed, fr, rr, pr, cr):
    """randomize_kernel's values of global env ``genv``: (payload, com[3], friction, restitution), float32.  The span
    is the float32 difference of the float32 range ends."""
    f = np.float32
    a = philox(genv, 0, RNG_INIT << 16, 0, seed)
    b = philox(genv, 0, RNG_INIT << 16, 1, seed)
    span = lambda r: f(f(r[1]) - f(r[0]))
    payload = draw32(u01(a[0]), span(pr), pr[0])
    com = np.array([draw32(u01(a[1 + k]), span(cr), cr[0]) for k in range(3)], f)
    return payload, com, draw32(u01(b[0]), span(fr), fr[0]), draw32(u01(b[1]), span(rr), rr[0])


def reset_uniforms(genv, count, seed):
    """reset_kernel's five uniforms (motor strength, Kp, Kd, x, y) of global env ``genv`` at its ``count``-th reset."""
    r = philox(genv, count, RNG_RESET << 16, 0, seed)
    r2 = philox(genv, count, RNG_RESET << 16, 1, seed)
    return np.array([u01(r[0]), u01(r[1]), u01(r[2]), u01(r[3]), u01(r2[0])], np.float32)


def terrain_level_draw(genv, step_counter, seed, max_level):
    """terrain_curriculum_kernel's wrap-around level: floor(word * max_level / 2^32), the counter's high word in the
    key."""
    step_counter = int(step_counter)
    r = philox(genv, step_counter & M32, ((RNG_TERRAIN << 16) ^ (step_counter >> 32)) & M32, 0, seed)
    return (r[0] * int(max_level)) >> 32


# ---------------------------------------------------------------------------------------------------------------
# The draws of the env step kernel and of the act kernels (csrc/lrl_env_step.h, observe_kernel, csrc/lrl_ppo.hip)
# ---------------------------------------------------------------------------------------------------------------
def step_key(stream, counter):
    """Counter words 1 and 2 of a per-step draw: the counter's low word, and (stream << 16) ^ its high word."""
    counter = int(counter)
    return counter & M32, ((stream << 16) ^ (counter >> 32)) & M32


def obs_noise_uniforms(genv, step_counter, seed, num_obs):
    """The observation row's noise uniforms of global env ``genv`` at ``step_counter`` (the value after lrl_sim_step's
    increment): entry i is word i & 3 of block i >> 2 on stream RNG_OBS_NOISE.  float32 [num_obs]."""
    c1, c2 = step_key(RNG_OBS_NOISE, step_counter)
    blocks = [philox(genv, c1, c2, b, seed) for b in range((num_obs + 3) >> 2)]
    return np.array([u01(blocks[i >> 2][i & 3]) for i in range(num_obs)], np.float32)


def push_uniforms(genv, step_counter, seed):
    """_push_robots' x and y uniforms: words 0 and 1 of block 0 on stream RNG_PUSH.  float32 [2]."""
    c1, c2 = step_key(RNG_PUSH, step_counter)
    r = philox(genv, c1, c2, 0, seed)
    return np.array([u01(r[0]), u01(r[1])], np.float32)


def dr_uniforms(genv, step_counter, seed, on_ms, on_kp, on_kd):
    """The per-step redraw's uniforms (motor strength, Kp, Kd) and the word each one took: words of block 0 on stream
    RNG_DR handed out in that order to the switches that are on; a switch that is off consumes no word (NaN, -1)."""
    c1, c2 = step_key(RNG_DR, step_counter)
    r = philox(genv, c1, c2, 0, seed)
    u, word = np.full(3, np.nan, np.float32), np.full(3, -1, np.int64)
    k = 0
    for i, on in enumerate((on_ms, on_kp, on_kd)):
        if on:
            u[i], word[i] = u01(r[k]), k
            k += 1
    return u, word


TWO_PI_F32 = np.float32(6.283185307179586)
U1_FLOOR = np.float32(1e-7)


def box_muller(u1, u2, odd):
    """Box-Muller in float64 from float32 uniforms (arrays or scalars): u1 clamped from below at float32(1e-7), the
    angle float32(2 pi) * u2 rounded once to float32 as the kernels round it; rad = sqrt(-2 ln u1), the even member of
    a pair takes rad cos, the odd one rad sin.  Returns (normal, rad)."""
    u1 = np.maximum(np.asarray(u1, np.float32), U1_FLOOR)
    th = (TWO_PI_F32 * np.asarray(u2, np.float32)).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return np.where(odd, rad * np.sin(th), rad * np.cos(th)), rad


def policy_normals(grow, counter, seed, na):
    """The act kernels' policy noise of global row ``grow`` at act counter ``counter``: action j draws from words 0
    and 1 of block j >> 1 on stream RNG_POLICY (a pair of actions shares a block).  float64 (normals [na], rad [na])."""
    c1, c2 = step_key(RNG_POLICY, counter)
    blocks = [philox(grow, c1, c2, b, seed) for b in range((na + 1) >> 1)]
    j = np.arange(na)
    u1 = np.array([u01(blocks[i >> 1][0]) for i in j], np.float32)
    u2 = np.array([u01(blocks[i >> 1][1]) for i in j], np.float32)
    return box_muller(u1, u2, (j & 1) == 1)


def policy_noise_bound(rad, e_ref, mu_over_sd=0.0):
    """The bar on |(a - mu) / sd - e_ref|: 8 x 2^-24 rad (logf, sqrtf and sinf / cosf at 2 ulp each plus the product's
    rounding, all relative to the radius) + 4 x 2^-24 (|mu| / sd + |e_ref|) (the roundings of mu + sd e and of the
    subtraction that recovers the noise)."""
    return 2.0 ** -24 * (8.0 * np.asarray(rad) + 4.0 * (np.abs(mu_over_sd) + np.abs(e_ref)))


def log_prob_terms(a, mu, sd):
    """Per action, in float64 from the given values: the Gaussian log-density and the magnitude sum d^2 / (2 sd^2) +
    |ln sd| + ln sqrt(2 pi) that its float32 evaluation's error scales with."""
    a, mu, sd = (np.asarray(x, np.float64) for x in (a, mu, sd))
    q = (a - mu) ** 2 / (2.0 * sd * sd)
    half_log_2pi = 0.5 * np.log(2.0 * np.pi)
    return -q - np.log(sd) - half_log_2pi, q + np.abs(np.log(sd)) + half_log_2pi


# the same generator on numpy uint64 arrays: for searches over keys and for row counts where the integer form is slow
def philox_v(c0, c1, c2, c3, seed):
    """``philox`` on broadcastable integer arrays: uint32 words [..., 4]."""
    m = np.uint64(M32)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) & m for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(int(seed) & M32), np.uint64((int(seed) >> 32) & M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u01_v(x):
    """``u01`` on arrays."""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def policy_normals_rows(grows, counter, seed, na):
    """``policy_normals`` of many rows at once through ``philox_v``: float64 (normals [rows, na], rad [rows, na])."""
    c1, c2 = step_key(RNG_POLICY, counter)
    j = np.arange(na)
    w = philox_v(np.asarray(grows, np.int64)[:, None] & M32, c1, c2, (j >> 1)[None, :], seed)
    return box_muller(u01_v(w[..., 0]), u01_v(w[..., 1]), ((j & 1) == 1)[None, :])


# ---------------------------------------------------------------------------------------------------------------
# Forward kinematics of the robot table
# ---------------------------------------------------------------------------------------------------------------
def quat_to_mat(q, dtype=np.float64):
    """Rotation matrix of the quaternion (x, y, z, w), normalised first."""
    q = np.asarray(q, dtype)
    x, y, z, w = q / np.sqrt(np.sum(q * q, dtype=dtype))
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype)


def axis_angle_mat(axis, th, dtype=np.float64):
    """Rodrigues: I + sin(th) [a] + (1 - cos(th)) [a]^2 for the unit axis a."""
    a = np.asarray(axis, dtype)
    a = a / np.sqrt(np.sum(a * a, dtype=dtype))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype)
    th = dtype(th)
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (dtype(1) - np.cos(th)) * (K @ K)


def _hom(R, p, dtype):
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = R
    T[:3, 3] = p
    return T


def body_frames(model, p, R, q, dtype=np.float64):
    """Homogeneous world transforms [B, 4, 4] of every body: base (p, R), then per leg the chain
    Trans(joint_xyz) Rot(joint_quat) Rot(joint_axis, q) of hip, thigh and calf; link 3 is the calf's frame moved to
    foot_xyz."""
    q = np.asarray(q, dtype)
    Tb = _hom(np.asarray(R, dtype), np.asarray(p, dtype), dtype)
    chain = {}
    for leg in range(4):
        T = Tb
        for j in range(3):
            Rj = quat_to_mat(model["joint_quat"][leg][j], dtype) @ axis_angle_mat(model["joint_axis"][leg][j],
                                                                                  q[3 * leg + j], dtype)
            T = T @ _hom(Rj, np.asarray(model["joint_xyz"][leg][j], dtype), dtype)
            chain[leg, j] = T
        chain[leg, 3] = T @ _hom(np.eye(3, dtype=dtype), np.asarray(model["foot_xyz"][leg], dtype), dtype)
    out = np.empty((len(model["body_leg"]), 4, 4), dtype)
    for b, (leg, link) in enumerate(zip(model["body_leg"], model["body_link"])):
        out[b] = Tb if leg < 0 else chain[leg, link]
    return out


def fk(model, root, com, q, qd, dtype=np.float64):
    """Rigid-body state of one env from the robot table (``joint_xyz``, ``joint_quat`` xyzw, ``joint_axis``,
    ``foot_xyz``, ``body_leg``, ``body_link``): per body the origin [B, 3], the rotation matrix [B, 3, 3], the linear
    velocity of the origin [B, 3] and the angular velocity [B, 3], all in the world frame.

    ``root`` = (position, quaternion xyzw, V, W): V is the velocity of the base's centre of mass, which sits at the
    displacement ``com`` (base frame) from the base origin, so the origin moves at V - W x (R com).  Positions and
    rotations come from ``body_frames``; the velocities are the textbook recursion over the same chain: a joint adds
    qd times its world axis to the angular velocity, and a child origin at offset r from its parent's moves at
    v + w x r."""
    root = np.asarray(root, dtype)
    return fk_mat(model, root[0:3], quat_to_mat(root[3:7], dtype), root[7:10], root[10:13], com, q, qd, dtype)


def _cross(a, b):
    """a x b of two 3-vectors, the products and differences np.cross takes, without its axis handling."""
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def fk_mat(model, p, R, V, W, com, q, qd, dtype=np.float64):
    """``fk`` from the base origin ``p``, the base rotation matrix ``R`` (base to world) and the world velocities V
    (of the base's centre of mass) and W."""
    p, R, V, W, com, q, qd = (np.asarray(a, dtype) for a in (p, R, V, W, com, q, qd))
    T = body_frames(model, p, R, q, dtype)
    v0 = V - _cross(W, R @ com)
    B = T.shape[0]
    pos, rot = T[:, :3, 3].copy(), T[:, :3, :3].copy()
    vel, ang = np.empty((B, 3), dtype), np.empty((B, 3), dtype)
    index = {(leg, link): b for b, (leg, link) in enumerate(zip(model["body_leg"], model["body_link"]))}
    done = {}
    for leg in range(4):
        o, v, w = p, v0, W
        Rp = R
        for j in range(3):
            Rj = Rp @ quat_to_mat(model["joint_quat"][leg][j], dtype) @ axis_angle_mat(
                model["joint_axis"][leg][j], q[3 * leg + j], dtype)
            r = Rp @ np.asarray(model["joint_xyz"][leg][j], dtype)
            a = np.asarray(model["joint_axis"][leg][j], dtype)
            a = a / np.sqrt(np.sum(a * a, dtype=dtype))
            v = v + _cross(w, r)
            w = w + qd[3 * leg + j] * (Rj @ a)
            o, Rp = o + r, Rj
            done[leg, j] = (v, w)
        done[leg, 3] = (v + _cross(w, Rp @ np.asarray(model["foot_xyz"][leg], dtype)), w)
    for (leg, link), b in index.items():
        vel[b], ang[b] = (v0, W) if leg < 0 else done[leg, link]
    return pos, rot, vel, ang


def rot_exp(w, dtype=np.float64):
    """exp([w]): the rotation by |w| about w."""
    th = float(np.linalg.norm(w))
    return np.eye(3, dtype=dtype) if th == 0.0 else axis_angle_mat(np.asarray(w) / th, th, dtype)


def quat_mat_branch(R):
    """Which branch the usual matrix-to-quaternion conversion takes for ``R`` (0: trace > 0; 1, 2, 3: the x, y, z
    diagonal entry is the largest) and how far R is from the nearest boundary between branches (the trace from 0, or
    the largest diagonal entry from the runner-up)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        return 0, t
    d = np.array([R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(d))
    return 1 + k, min(-t, d[k] - np.max(np.delete(d, k)))


# ---------------------------------------------------------------------------------------------------------------
# The small references
# ---------------------------------------------------------------------------------------------------------------
def due(episode_length, interval):
    """Envs due for command resampling: (episode_length + 1) % interval == 0, every env when interval == 1."""
    return (np.asarray(episode_length, np.int64) + 1) % int(interval) == 0


def env_list(mode, reset, episode_length, interval):
    """lrl_sim_env_lists: ascending ids of the set reset flags (mode 0) or of the due envs (mode 1)."""
    return np.flatnonzero(np.asarray(reset) != 0 if mode == 0 else due(episode_length, interval)).astype(np.int32)


def step_code(reset, episode_length, interval):
    """Per env: bit 0 the reset flag, bit 1 due for resampling, as a float32."""
    return ((np.asarray(reset) != 0).astype(np.int64) | (due(episode_length, interval).astype(np.int64) << 1)) \
        .astype(np.float32)


def shift_history(hist, obs):
    """HistoryWrapper: every row becomes concat(old[NO:], obs)."""
    return np.concatenate([hist[:, obs.shape[1]:], obs], axis=1)


def row_means(table, ids):
    """float64 mean of every row over the columns ``ids`` (NaN for an empty list), and sum |x| / n for the bound."""
    x = np.asarray(table, np.float64)[:, np.asarray(ids, np.int64)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return x.sum(1) / x.shape[1], np.abs(x).sum(1) / x.shape[1]
