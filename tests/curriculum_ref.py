"""The command curriculum's resample as numpy itself performs it: the reference of tests/test_curriculum_dev_gpu.py.

Plain numpy in float64 around a real ``np.random.RandomState``; nothing of ``lrl.curriculum`` is imported and none of
the device kernel's restatements (Mersenne twister, pairwise sum, cdf search, counted adds) appears here.  Written from
the behaviour the header of csrc/lrl_curriculum_dev.hip cites:

* the grid: one ``np.linspace`` axis per key, ``meshgrid(indexing='ij')`` flattened to [3, nbins];
  ``half = bin_size / 2`` with ``bin_size = axis[1] - axis[0]``.  A one-point axis has no ``axis[1]``: there the cited
  code (and ``lrl.curriculum``) raises IndexError, so such a grid exists only with ``bin_sizes`` given by the caller,
  which is how the device descriptor carries ``half`` anyway;
* ``update``: the fancy assignment of the episode rewards, ``ok = (lin > thr_lin) * (ang > thr_ang)``, the clipped
  +0.2 on ``weights[bins[ok]]``, then a Python loop over the successful entries, each adding a clipped 0.2 to every bin
  whose three grid values lie in [c - r, c + r];
* ``sample``: ``rng.choice(nbins, n, p=w / w.sum())``, then one ``rng.uniform(cent + half, cent - half)`` over [n, 3];
* ``resample``: _resample_commands' writes around them (commands[ids, :3] in float32, the |xy| > 0.2 mask as the
  multiplication by the 0 / 1 mask that the cited code does, so a masked negative component is -0.0;
  command_sums[:, ids] = 0; the env bins), and reset_idx's log values with ``log_area``.

The comparison rule of ``ok``: the rewards are float32 arrays and the thresholds Python floats; the threshold is cast to
float32 and the comparison is made in float32 (NumPy 2's rule for a Python scalar against a float32 array).  It is
written out below (the threshold cast to the reward array's type) so that it does not rest on the installed numpy's promotion.
"""
import warnings

import numpy as np

F32 = np.float32
# RandomState.choice's messages (numpy 2.2.6: zero or inf weights make p NaN; a negative weight a negative p) and the
# code lrl_dev_curriculum.state[2] reports for each
ERROR_CODES = {"probabilities contain NaN": 1, "probabilities are not non-negative": 2,
               "probabilities do not sum to 1": 3}


class CurriculumRef:
    def __init__(self, ranges, num_envs, n_sums, key=None, pos=624, seed=0, bin_sizes=None):
        """ranges: three (low, high, points); key / pos: the MT19937 state (default: RandomState(seed)'s key)."""
        self.axes = [np.linspace(*r) for r in ranges]
        if bin_sizes is None:
            bin_sizes = [a[1] - a[0] for a in self.axes]  # IndexError on a one-point axis, as the cited code
        self.bin_sizes = np.array(bin_sizes, np.float64)
        self.half = self.bin_sizes / 2
        self.shape = tuple(len(a) for a in self.axes)
        self.grid = np.stack(np.meshgrid(*self.axes, indexing="ij")).reshape(3, -1)
        self.nb = self.grid.shape[1]
        self.rng = np.random.RandomState(seed)
        if key is not None or pos != 624:
            key = self.rng.get_state()[1] if key is None else key
            self.rng.set_state(("MT19937", np.asarray(key, np.uint32), int(pos)))
        self.weights = np.zeros(self.nb)
        self.episode_reward_lin = np.zeros(self.nb)
        self.episode_reward_ang = np.zeros(self.nb)
        self.env_bins = np.zeros(num_envs, np.int64)
        self.env_bins_f = np.zeros(num_envs, F32)
        self.command_area = np.zeros(1)
        self.commands = np.zeros((num_envs, 4), F32)
        self.command_sums = np.zeros((n_sums, num_envs), F32)
        self.cdf = None  # p.cumsum() / cumsum[-1] of the last successful sample
        self.error = None  # the message of the last choice that raised

    @property
    def mt(self):
        st = self.rng.get_state()
        return np.array(st[1], np.uint32), int(st[2])

    def update(self, old_bins, lin32, ang32, lin_thr, ang_thr, local_range):
        """curriculum.py:105-115 as written.  Returns the successful entries' bins (in list order)."""
        self.episode_reward_lin[old_bins] = lin32
        self.episode_reward_ang[old_bins] = ang32
        # the threshold cast to the rewards' type: float32 rewards (every resample) are compared in float32
        ok = (lin32 > lin32.dtype.type(lin_thr)) * (ang32 > ang32.dtype.type(ang_thr))
        w = self.weights
        counts, clipped = np.zeros(self.nb, np.int64), int((w[old_bins[ok]] + 0.2 > 1).sum())
        w[old_bins[ok]] = np.clip(w[old_bins[ok]] + 0.2, 0, 1)
        for b in old_bins[ok]:
            c = self.grid[:, b]
            inside = np.logical_and(self.grid >= (c - local_range)[:, None],
                                    self.grid <= (c + local_range)[:, None]).all(axis=0)
            idx = inside.nonzero()[0]
            counts[idx] += 1
            clipped += int((w[idx] + 0.2 > 1).sum())
            w[idx] = np.clip(w[idx] + 0.2, 0, 1)
        # (for the tests' coverage conditions: the neighbourhood adds per bin, and the adds that the clip cut)
        self.last_update = dict(counts=counts, clipped=clipped)
        return old_bins[ok]

    def sample(self, n):
        w = self.weights
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = w / w.sum()
        bins = self.rng.choice(self.nb, n, p=p)
        cs = p.cumsum()
        self.cdf = cs / cs[-1]
        cent = self.grid.T[bins]
        return self.rng.uniform(cent + self.half, cent - self.half), bins

    def resample(self, ids, count, nmax, ep_len, row_lin, row_ang, lin_thr, ang_thr, local_range, update, log_area,
                 prev_bins_f=None, prev_area=None):
        """One lrl_sim_curriculum_resample_dev call on this state.  Returns what happened: n, the successful
        entries' bins (None without update), the error message (None when the sample succeeded), the listed envs' old
        bins and float32 rewards, and the float64 norms the mask compared with 0.2."""
        n = min(int(count), int(nmax))
        if n <= 0:  # lrl.h: with log_area, an empty batch copies the previous step's log values when they are given
            if log_area and prev_bins_f is not None:
                self.env_bins_f[:] = prev_bins_f
                if prev_area is not None:
                    self.command_area[0] = prev_area
            return dict(n=0, centres=None, error=None)
        ids = np.asarray(ids[:n], np.int64)
        old = self.env_bins[ids]
        lin = self.command_sums[row_lin, ids] / F32(ep_len)
        ang = self.command_sums[row_ang, ids] / F32(ep_len)
        assert lin.dtype == F32 and ang.dtype == F32
        centres = self.update(old, lin, ang, lin_thr, ang_thr, local_range) if update else None
        try:
            cmds, bins = self.sample(n)
        except ValueError as e:  # choice raised before any draw: the generator and every output stay
            self.error = str(e)
            self.cdf = None
            return dict(n=n, centres=centres, error=self.error, old=old, lin=lin, ang=ang)
        self.error = None
        c32 = cmds.astype(F32)
        norm = np.linalg.norm(c32[:, :2].astype(np.float64), axis=1)  # float64 norm of the float32 commands
        c32[:, :2] *= (norm > 0.2)[:, None]
        self.commands[ids, :3] = c32
        self.command_sums[:, ids] = 0
        self.env_bins[ids] = bins
        if log_area:
            self.command_area[0] = np.sum(self.weights) / self.nb
            self.env_bins_f[:] = self.env_bins.astype(F32)
        return dict(n=n, centres=centres, error=None, norm=norm, old=old, lin=lin, ang=ang)

