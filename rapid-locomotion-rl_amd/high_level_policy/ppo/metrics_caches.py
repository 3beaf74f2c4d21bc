from lrl.hlp.metrics_caches import DistCache, SlotCache  # noqa: F401
