"""High-level (navigation) policy learning (high_level_policy/ppo/*): a plain tanh MLP actor-critic trained by PPO
over ``lrl.high_level.HighLevelControlWrapper``.

The reference builds this network with ``USE_LATENT = False``: the actor and the critic read the 14 observations
alone, and there is no env-factor encoder and no adaptation module.  The native side is the ``plain`` / tanh form of
the ``lrl_ppo_*`` calls (include/lrl.h); the classes here derive from ``lrl.ppo``'s and change only what that form
changes.
"""
import os

USE_LATENT = False  # the latent (teacher / student) form of the high-level policy is not implemented
HLP_ROOT_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.realpath(__file__))))

from .actor_critic import AC_Args, ActorCritic  # noqa: E402,F401
from .ppo import PPO, PPO_Args  # noqa: E402,F401
from .rollout_storage import RolloutStorage  # noqa: E402,F401
from .runner import Runner, RunnerArgs  # noqa: E402,F401
