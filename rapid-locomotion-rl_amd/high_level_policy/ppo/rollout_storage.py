"""high_level_policy/ppo/rollout_storage.py surface."""
from lrl.hlp.rollout_storage import RolloutStorage  # noqa: F401
