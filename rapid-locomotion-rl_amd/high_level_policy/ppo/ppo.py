from lrl.hlp.ppo import PPO, PPO_Args  # noqa: F401
