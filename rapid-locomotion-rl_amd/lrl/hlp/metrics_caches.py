"""Running-mean metric caches of the high-level runner (high_level_policy/ppo/metrics_caches.py): ``caches`` is the
module-level pair the reference exposes as ``high_level_policy.ppo.caches``.  The navigation wrapper reports no
curriculum, so nothing logs into them during ``Runner.learn``; they exist for the reference's import surface."""
from collections import defaultdict

import numpy as np


class _MeanCache:
    """key -> running mean of the logged values (``key@counts`` holds the sample count); a summary empties it."""

    def _zero(self):
        return 0

    def __init__(self):
        self.cache = defaultdict(self._zero)

    def _log(self, sel, key_vals):
        for k, v in key_vals.items():
            cnt, cur = self.cache[k + "@counts"], self.cache[k]
            if sel is None:
                n = cnt + 1
                self.cache[k + "@counts"], self.cache[k] = n, (v + cnt * cur) / n
            else:
                n = cnt[sel] + 1
                cur[sel] = (v + cnt[sel] * cur[sel]) / n
                cnt[sel] = n

    def get_summary(self):
        out = {k: v for k, v in self.cache.items() if not k.endswith("@counts")}
        self.cache.clear()
        return out


class DistCache(_MeanCache):
    def log(self, **key_vals):
        self._log(None, key_vals)


class SlotCache(_MeanCache):
    """``n`` slots per key; ``log(slots, key=values)`` updates the named slots (all of them when ``slots`` is None)."""

    def __init__(self, n):
        self.n = n
        super().__init__()

    def _zero(self):
        return np.zeros([self.n])

    def log(self, slots=None, **key_vals):
        self._log(range(self.n) if slots is None else slots, key_vals)


class DataCaches:
    def __init__(self, curriculum_bins):
        self.slot_cache = SlotCache(curriculum_bins)
        self.dist_cache = DistCache()


caches = DataCaches(1)
