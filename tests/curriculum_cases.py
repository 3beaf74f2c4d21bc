"""The inputs of tests/test_curriculum_dev_gpu.py: grids, call chains and the coverage they must reach.

A chain is a list of lrl_sim_curriculum_resample_dev calls on one sim; every call names the whole pre-call content of
the buffers the test fills (commands, command sums, env bins, log buffers) and its arguments.  ``run_chain`` plays a
chain on a ``curriculum_ref.CurriculumRef`` and hands each call, the reference's state before and after it, to a hook
(the device comparison).  tests/test_curriculum_ref.py plays the same chains without a hook and asserts the coverage
conditions on the reference alone, so a device run cannot pass on inputs that miss a case.
"""
import numpy as np

import curriculum_ref as cr

F32 = np.float32
LIN_THR, ANG_THR = 0.3, 0.2  # not float32 values: float32(0.3) > 0.3 and float32(0.2) > 0.2
MAX_PASSING = 300            # the reference's neighbourhood loop is Python: successful entries per call
BATCHES = (1, 78, 79, 256, 1024, 1025, 4096)  # 78 envs draw 624 words, one MT19937 block exactly
POSITIONS = (624, 0, 620, 623)                # a fresh RandomState; 623: a double's two words straddle the twist
EP_LENS = (25, 7, 1001)

# (low, high, points) per axis; bin_sizes only where a one-point axis leaves axis[1] - axis[0] undefined.  The xy cells
# straddle 0, so that norms on both sides of 0.2 occur.
GRIDS = {
    "1x1x1": dict(ranges=((0.1, 0.1, 1), (0.1, 0.1, 1), (0.0, 0.0, 1)), bin_sizes=(0.5, 0.5, 1.0)),
    "2x1x3": dict(ranges=((-0.3, 0.3, 2), (0.0, 0.0, 1), (-1.0, 1.0, 3)), bin_sizes=(0.6, 0.5, 1.0)),
    "5x2x11": dict(ranges=((-1.0, 1.0, 5), (-0.6, 0.6, 2), (-1.0, 1.0, 11))),
    "8x2x8": dict(ranges=((-0.7, 0.7, 8), (-0.3, 0.3, 2), (-3.5, 3.5, 8))),
    "43x1x3": dict(ranges=((-10.5, 10.5, 43), (0.0, 0.0, 1), (-1.0, 1.0, 3)), bin_sizes=(0.5, 0.6, 1.0)),
    "51x2x51": dict(ranges=((-10.0, 10.0, 51), (-0.6, 0.6, 2), (-10.0, 10.0, 51))),
    "10x2x389": dict(ranges=((-0.9, 0.9, 10), (-0.3, 0.3, 2), (-40.0, 40.0, 389))),
}
REFUSED_GRID = dict(ranges=((-3.0, 3.0, 31), (0.0, 0.0, 1), (-25.0, 25.0, 251)), bin_sizes=(0.2, 0.6, 0.2))
# RandomState seeds of the chains (+ the variant), chosen so that no drawn xy norm lies within 1e-6 of 0.2
SEEDS = dict({k: 1000 for k in GRIDS}, **{"1x1x1": 2000, "2x1x3": 6000})
MAX_BINS = 7780  # the launcher's limit: 16 nb + 2496 bytes of dynamic LDS <= 124 KB


def ladder():
    """The weights that repeated clipped +0.2 adds reach from 0: 0, 0.2, 0.4, 0.6000000000000001, 0.8, 1.0."""
    w, out = 0.0, [0.0]
    for _ in range(5):
        w = float(np.clip(w + 0.2, 0, 1))
        out.append(w)
    return np.array(out)


def pairwise_tree(n):
    """The recursion of numpy's pairwise sum over n contiguous float64, level by level: (levels, widest level, leaf
    lengths); a node of more than 128 elements splits at n2 = n / 2 - (n / 2) % 8."""
    level, depth, widest, leaves = [n], 0, 1, []
    while level:
        depth += 1
        widest = max(widest, len(level))
        nxt = []
        for m in level:
            if m <= 128:
                leaves.append(m)
            else:
                n2 = m // 2
                n2 -= n2 % 8
                nxt += [n2, m - n2]
        level = nxt
    return depth, widest, leaves


def make_ref(gname, num_envs, n_sums, pos=624, seed=0):
    g = GRIDS[gname] if isinstance(gname, str) else gname
    return cr.CurriculumRef(g["ranges"], num_envs, n_sums, pos=pos, seed=seed, bin_sizes=g.get("bin_sizes"))


def spacing_range(ref):
    """A local_range equal to the spacing of the longest axis (0.25 on the one-bin grid): membership of the next grid
    value rests on >= / <= between rounded float64 values."""
    a = max(ref.axes, key=len)
    return float(a[1] - a[0]) if len(a) > 1 else 0.25


def sum_for(target, ep_len):
    """A float32 sum s with float32(s / ep_len) == target exactly, or None when the division skips target."""
    s0 = F32(F32(target) * F32(ep_len))
    cand = [s0]
    up = down = s0
    for _ in range(6):
        up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
        cand += [up, down]
    for s in cand:
        if F32(s) / F32(ep_len) == F32(target):
            return F32(s)
    return None


def threshold_rewards():
    """(name, lin, ang) of the six entries that sit on a threshold: float32(thr) itself (fails a strict float32
    comparison, passes a float64 one and a >=), its float32 neighbour below (fails) and above (passes); the other
    reward passes clearly."""
    out = []
    for which, thr, other in (("lin", LIN_THR, 0.35), ("ang", ANG_THR, 0.5)):
        t = F32(thr)
        for tag, v in (("at", t), ("below", np.nextafter(t, F32(0))), ("above", np.nextafter(t, F32(1)))):
            out.append((f"{which} {tag}", v, F32(other)) if which == "lin" else (f"{which} {tag}", F32(other), v))
    return out


def corners(shape):
    nx, ny, nz = shape
    return sorted({(x * ny + y) * nz + z for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)})


# the calls of a chain: (update, log_area, id list, count, special)
PLAN = (
    (1, 0, "perm", "exact", "stale cdf"),   # state[0] = 0 and a poisoned cdf buffer: recomputed
    (1, 1, "full", "less", None),           # entries past the count are other envs' ids: ignored
    (0, 0, "upper", "more", None),          # the count above nmax: clamped
    (0, 1, "perm", "less", None),
    (1, 1, "upper", "exact", "all fail"),   # nothing passes: the cdf buffer and state[0] = 1 stay
    (1, 0, "full", "more", None),
    (0, 0, "perm", "empty", None),          # count 0: nothing changes, the generator included
    (0, 1, "perm", "empty", "prev"),        # count 0 with log_area: the previous log values are copied
    (0, 1, "perm", "empty", "no prev"),     # ... or, with null prevs, the buffers stay
    (1, 1, "perm", "exact", None),
    (0, 0, "perm", "exact", "stale cdf"),
)


def chain(gname, n, pos, variant, n_sums, pair):
    """The calls of one chain (a generator of dicts) on grid ``gname`` with nominal batch size n, starting at MT
    position pos.  variant: 0 random ladder weights, 1 every weight 1.0, 2 weights near the origin only.
    pair: the env's (tracking_lin_vel, tracking_ang_vel) sum rows."""
    names = list(GRIDS)
    rng = np.random.default_rng([names.index(gname), n, pos, variant])
    ref0 = make_ref(gname, 1, 1)
    nb, shape = ref0.nb, ref0.shape
    N = n if n >= 4096 else n + n // 2 + 3
    sub = min(n, 2500) if N == n and n > 1 else n
    lad = ladder()
    if variant == 1:
        weights = np.ones(nb)
    else:
        weights = lad[rng.integers(0, 6, nb)] * (rng.random(nb) < (0.5 if variant == 0 else 0.05))
        near = (np.abs(ref0.grid[0]) <= 0.5) & (np.abs(ref0.grid[2]) <= 1.0)
        weights[near] = lad[rng.integers(1, 6, int(near.sum()))]
        k = min(nb, 6)  # every value of the ladder over a grid's chains, however small the grid
        weights[:k] = np.roll(lad, chains_of(gname).index((n, pos, variant)))[:k]
        if not weights.any():
            weights[0] = 0.2  # (never all zero)
    yield dict(kind="init", N=N, weights=weights, pos=pos, seed=SEEDS[gname] + variant)
    ranges = [0.5, 0.1, 1.0, spacing_range(ref0)]
    corner_bins = corners(shape)
    thr = threshold_rewards()
    k_upd = variant
    for k, (update, log_area, how, count_how, special) in enumerate(PLAN):
        if how == "perm":
            ids = rng.permutation(N)[:sub]
        elif how == "full":
            ids = np.arange(N)
        else:
            ids = N // 2 + rng.permutation(N - N // 2)[:min(n, N - N // 2)]
        ids = ids.astype(np.int32)
        L = len(ids)
        if count_how == "exact":
            count = nmax = L
        elif count_how == "less":
            count, nmax = (L - min(5, L // 2), L)
        elif count_how == "more":
            count, nmax = (L + 7 if k % 2 else 2 ** 31 - 1), L
        else:
            count, nmax = 0, L
        m = min(count, nmax)
        ep_len = EP_LENS[(k + variant) % 3]
        rows = pair if k % 2 == 0 else (n_sums - 1, 0)
        env_bins = rng.integers(0, nb, N)
        sums = rng.uniform(-50, 50, (n_sums, N)).astype(F32)
        lin = rng.uniform(0.0, 0.6, m).astype(F32)
        ang = rng.uniform(0.0, 0.4, m).astype(F32)
        placed, e = {}, 0
        if update and m:
            if special == "all fail":
                lin = rng.uniform(0.0, 0.29, m).astype(F32)
            listed = ids[:m]
            if m >= len(corner_bins) + 3:  # old bins at every corner of the grid, all passing
                env_bins[listed[:len(corner_bins)]] = corner_bins
                if special != "all fail":
                    lin[:len(corner_bins)], ang[:len(corner_bins)] = 0.5, 0.35
                e = len(corner_bins)
            if m - e >= 3:  # one bin held by several listed envs, rewards alternating pass / fail, all different
                d = min(max(3, (m - e) // 3), 40)
                env_bins[listed[e:e + d]] = env_bins[listed[e]]
                if special != "all fail":
                    lin[e:e + d] = np.where(np.arange(d) % 2 == 0, 0.4, 0.1) + rng.uniform(0, 0.05, d)
                    ang[e:e + d] = 0.3 + rng.uniform(0, 0.05, d)
                e += d
            if special != "all fail":  # at most MAX_PASSING successful entries
                passing = np.flatnonzero((lin > 0.29) & (ang > 0.19))
                for i in passing[MAX_PASSING:]:
                    lin[i] = 0.01
        s_lin, s_ang = (lin * F32(ep_len)).astype(F32), (ang * F32(ep_len)).astype(F32)
        if update and m and special != "all fail":  # the threshold entries, where the sums exist and room is left
            free = list(range(e, m))
            for (name, tl, ta) in thr:
                a, b = sum_for(tl, ep_len), sum_for(ta, ep_len)
                if a is None or b is None or not free:
                    continue
                i = free.pop()
                s_lin[i], s_ang[i] = a, b
                placed[name] = i
        sums[rows[0], ids[:m]] = s_lin
        if rows[1] != rows[0]:
            sums[rows[1], ids[:m]] = s_ang
        yield dict(kind="call", k=k, ids=ids, count=count, nmax=nmax, ep_len=ep_len, rows=rows, update=update,
                   log_area=log_area, special=special, placed=placed,
                   local_range=ranges[k_upd % 4] if update else 0.5,
                   env_bins=env_bins.astype(np.int64), sums=sums,
                   commands=rng.uniform(-9, 9, (N, 4)).astype(F32),
                   env_bins_f=rng.uniform(-9, 9, N).astype(F32), area=float(rng.uniform(2, 3)),
                   prev_bins_f=rng.uniform(10, 20, N).astype(F32), prev_area=float(rng.uniform(4, 5)))
        k_upd += update


def chains_of(gname):
    """(n, pos, variant) of the chains of one grid: every batch size at two starting positions (all four over the
    set, 78 envs from both block-aligned ones), the all-ones weights and the sparse weights at 256 envs."""
    g = list(GRIDS).index(gname)
    out = []
    for i, n in enumerate(BATCHES):
        for j in (0, 2):
            out.append((n, POSITIONS[(i + g + j) % 4], 0))
    out += [(78, 624, 0), (78, 0, 0), (1, 623, 0), (256, 623, 1), (256, 620, 2)]
    return sorted(set(out))


def load(ref, call):
    """The call's pre-call buffer contents into the reference."""
    ref.env_bins[:] = call["env_bins"]
    ref.command_sums[:] = call["sums"]
    ref.commands[:] = call["commands"]
    ref.env_bins_f[:] = call["env_bins_f"]
    ref.command_area[0] = call["area"]


def apply(ref, call):
    prev = call["special"] == "prev"
    return ref.resample(call["ids"], call["count"], call["nmax"], call["ep_len"], call["rows"][0], call["rows"][1],
                        LIN_THR, ANG_THR, call["local_range"], call["update"], call["log_area"],
                        prev_bins_f=call["prev_bins_f"] if prev else None,
                        prev_area=call["prev_area"] if prev else None)


class Coverage:
    """What a set of chains reached, gathered from the reference alone."""

    def __init__(self):
        self.masked = self.kept = 0
        self.mask_margin = np.inf
        self.double_add = self.clipped = self.all_ones_pass = self.last_wins_mix = False
        self.cut = [False, False, False]
        self.corner_bins = set()
        self.placed = set()
        self.weights_seen = set()
        self.combos = set()
        self.counts = set()
        self.lists = set()
        self.max_passing = 0
        self.batch = set()
        self.positions = set()
        self.stale = self.cached = 0

    def before(self, ref, call):
        self.w_before = ref.weights.copy()

    def after(self, ref, call, info):
        if info["n"] == 0:
            self.counts.add(("empty", call["log_area"], call["special"]))
            return
        self.batch.add(info["n"])
        self.combos.add((call["update"], call["log_area"]))
        if call["ids"].tolist() == list(range(len(ref.env_bins))):
            self.lists.add("full")
        else:
            self.lists.add("upper" if call["ids"].min() >= len(ref.env_bins) // 2 else "perm")
        self.counts.add("less" if call["count"] < call["nmax"] else "more" if call["count"] > call["nmax"] else "exact")
        if info["error"] is None:
            d = np.abs(info["norm"] - 0.2)
            self.mask_margin = min(self.mask_margin, d.min())
            self.masked += int((info["norm"] <= 0.2).sum())
            self.kept += int((info["norm"] > 0.2).sum())
        cen = info["centres"]
        if cen is None:
            return
        self.max_passing = max(self.max_passing, len(cen))
        if len(cen) == 0:
            self.cached += 1
            return
        w0 = self.w_before
        if (w0[cen] == 1.0).all():
            self.all_ones_pass = True
        r = call["local_range"]
        for b in cen:
            c = ref.grid[:, b]
            for d in range(3):  # the interval [c - r, c + r] reaches past an end of the axis
                if c[d] - r < ref.axes[d][0] or c[d] + r > ref.axes[d][-1]:
                    self.cut[d] = True
        if ref.last_update["counts"].max() >= 2:
            self.double_add = True
        if ref.last_update["clipped"] > 0:
            self.clipped = True
        old, lin, ang = info["old"], info["lin"], info["ang"]
        self.corner_bins |= set(old.tolist()) & set(corners(ref.shape))
        ok = (lin > F32(LIN_THR)) & (ang > F32(ANG_THR))
        for b in np.unique(old):
            sel = old == b
            if sel.sum() >= 3 and ok[sel].any() and not ok[sel].all() and len(set(lin[sel].tolist())) == sel.sum():
                self.last_wins_mix = True
        for name, tl, ta in threshold_rewards():
            i = call["placed"].get(name)
            if i is not None:
                assert lin[i] == tl and ang[i] == ta
                self.placed.add(name)


def run_chain(gname, n, pos, variant, n_sums, pair, hook=None, cover=None):
    """Plays a chain on a fresh reference.  hook(ref, call, phase, info): phase 'init' once, then 'before' / 'after'
    around every call ('before' sees the reference with the call's pre-call buffers loaded)."""
    ref = None
    for call in chain(gname, n, pos, variant, n_sums, pair):
        if call["kind"] == "init":
            ref = make_ref(gname, call["N"], n_sums, pos=call["pos"], seed=call["seed"])
            ref.weights[:] = call["weights"]
            if cover is not None:
                cover.positions.add(call["pos"])
                cover.weights_seen |= set(call["weights"].tolist())
            if hook:
                hook(ref, call, "init", None)
            continue
        load(ref, call)
        if cover is not None:
            cover.before(ref, call)
            if call["special"] == "stale cdf":
                cover.stale += 1
        if hook:
            hook(ref, call, "before", None)
        info = apply(ref, call)
        if cover is not None:
            cover.after(ref, call, info)
        if hook:
            hook(ref, call, "after", info)
    return ref
