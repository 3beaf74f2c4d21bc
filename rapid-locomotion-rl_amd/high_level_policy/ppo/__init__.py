"""``high_level_policy.ppo`` surface: Runner, RunnerArgs, ActorCritic, RolloutStorage, caches."""
from lrl.hlp.actor_critic import AC_Args, ActorCritic  # noqa: F401
from lrl.hlp.metrics_caches import DataCaches, caches  # noqa: F401
from lrl.hlp.rollout_storage import RolloutStorage  # noqa: F401
from lrl.hlp.runner import Runner, RunnerArgs  # noqa: F401
