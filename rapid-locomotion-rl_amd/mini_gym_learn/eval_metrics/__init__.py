"""``mini_gym_learn.eval_metrics`` surface: ``metrics.METRICS_FNS`` and ``domain_randomization.DR_SETTINGS`` / ``base_set``."""
