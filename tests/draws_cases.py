"""Shared by tests/test_draws_ref.py (CPU: the helpers of aux_ref.py and the oracle), tests/test_draws_gpu.py (the env
step kernel's and observe_kernel's own draws) and tests/test_policy_draws_gpu.py (the act kernels' policy noise): the
parameter blocks that make every draw visible, the keys, and the reference uniforms of a whole sim."""
import numpy as np

import aux_ref as ar

F32 = np.float32
SEED = 0x1234567089ABCDEF  # both key words non-zero
WRAP = (5 << 32) + 0xFFFFFFFF  # the step's increment wraps the low word and carries into the word XORed into the key
BIG_OFFSET = (1 << 31) + 5
# episode lengths before the step; after its increment: 12 (redraw and push), 3 (redraw), 4 (push), 1 (neither),
# 6 (redraw), 8 (push), 2 (neither) at rand_interval 3 and push_interval 4.  Env 0 draws everything (the n = 1 case).
EPLEN_POOL = np.array([11, 2, 3, 0, 5, 7, 1], np.int32)
RAND_INTERVAL, PUSH_INTERVAL = 3, 4


def copy_params(P):
    return type(P).from_buffer_copy(P)


def set_dr(B, ms, kp, kd, ms_range, kp_range, kd_range):
    """The redraw switches and ranges of a parameter block or an eval-group block; the span as build_params forms it
    (the python-float difference, rounded to float32 by the field)."""
    B.randomize_motor_strength, B.randomize_kp, B.randomize_kd = int(ms), int(kp), int(kd)
    for k, (f, r) in enumerate((("motor_strength_range", ms_range), ("kp_range", kp_range), ("kd_range", kd_range))):
        getattr(B, f)[0], getattr(B, f)[1] = r
        B.dr_span[k] = float(r[1]) - float(r[0])


def set_push(B, on, interval, vmax):
    B.push_robots, B.push_interval, B.push_lo, B.push_span = int(on), int(interval), -vmax, vmax - (-vmax)


def visible_params(P, ms=True, kp=True, kd=True, zero_noise=False):
    """A copy of ``P`` on which every draw of a step shows: a noise vector of distinct non-zero values over the whole
    row (the shipped one is zero on the commands and the actions), redraws every 3rd and pushes every 4th step of an
    episode.  clip_obs stays at its default."""
    Q = copy_params(P)
    assert Q.add_noise
    for i in range(Q.num_obs):
        Q.noise_vec[i] = 0.0 if zero_noise else 0.02 + 0.0005 * i
    Q.rand_interval = RAND_INTERVAL
    set_dr(Q, ms, kp, kd, (0.9, 1.1), (0.8, 1.3), (0.5, 1.5))
    set_push(Q, True, PUSH_INTERVAL, 0.5)
    return Q


def eval_block(G):
    """The eval group of the split sims: (kp, kd) against the train group's (ms, kd), ranges disjoint from
    ``visible_params``', another push interval and span."""
    set_dr(G, False, True, True, (0.4, 0.6), (1.5, 1.75), (2.0, 2.5))
    set_push(G, True, 3, 0.9)
    return G


def blocks_of(P, G, n, n_train):
    """Per env the block whose redraw / push fields it reads."""
    return [P if (G is None or e < n_train) else G for e in range(n)]


def due(blocks, rand_interval, eplen_before):
    """(redraw, push) masks of one step: episode_length + 1 a multiple of the interval."""
    L = np.asarray(eplen_before, np.int64) + 1
    redraw = (L % rand_interval == 0) if rand_interval > 0 else np.zeros(len(L), bool)
    push = np.array([bool(B.push_robots) and L[e] % max(B.push_interval, 1) == 0 for e, B in enumerate(blocks)])
    return redraw, push


def step_uniforms(blocks, num_obs, offset, counter, seed):
    """The reference uniforms of every env of a sim for the step whose counter (after the increment) is ``counter``:
    obs noise [n, NO], the redraw's uniforms [n, 3] with their word indices [n, 3], push uniforms [n, 2]."""
    n = len(blocks)
    noise = np.stack([ar.obs_noise_uniforms(offset + e, counter, seed, num_obs) for e in range(n)])
    dr = [ar.dr_uniforms(offset + e, counter, seed, B.randomize_motor_strength, B.randomize_kp, B.randomize_kd)
          for e, B in enumerate(blocks)]
    push = np.stack([ar.push_uniforms(offset + e, counter, seed) for e in range(n)])
    return noise, np.stack([d[0] for d in dr]), np.stack([d[1] for d in dr]), push


def injected_ms(dr_u):
    """The motor-strength column as lrl_sim_inject_uniforms takes it (0.5 where the env's group draws none)."""
    return np.nan_to_num(dr_u[:, 0], nan=0.5).astype(F32)


def gentle_heights(G, hs, vs):
    """Centimetre-high bumps on a G x G grid as int16 height samples (test_aux_gpu.set_gentle_terrain's map)."""
    i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    return np.round(0.05 * np.sin(0.7 * i * hs) * np.cos(0.5 * j * hs) / vs).astype(np.int16)


# ---- policy noise: (seed, counter, row_offset, n) of the act tests -------------------------------------------------
ACT_SEED = 0x1234567089ABCDEF
ACT_COUNTERS = (3, (7 << 32) | 9)
ACT_OFFSETS = (0, 64, (1 << 31) + 11)
# u01(word 0) == 0 for actions 2 and 3 of this global row at seed 11, counter 3 (test_draws_ref.py recomputes it)
CLAMP_SEED, CLAMP_COUNTER, CLAMP_ROW, CLAMP_BLOCK = 11, 3, 2473292, 1
# (n, counter, row_offset) per act path: every n, counter and offset appears with every path
ACT_CASES = [(1, ACT_COUNTERS[0], ACT_OFFSETS[2]), (37, ACT_COUNTERS[1], ACT_OFFSETS[0]),
             (300, ACT_COUNTERS[0], ACT_OFFSETS[1]), (37, ACT_COUNTERS[1], ACT_OFFSETS[2])]
STATS_N, STATS_COUNTER = 8192, 5


def act_keys():
    """Every (seed, counter, row_offset, n) the act tests draw with."""
    keys = [(ACT_SEED, c, ro, n) for n, c, ro in ACT_CASES]
    keys.append((CLAMP_SEED, CLAMP_COUNTER, CLAMP_ROW - 5, 16))
    keys.append((ACT_SEED, STATS_COUNTER, 0, STATS_N))
    return keys
