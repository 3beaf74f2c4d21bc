"""The high-level policy's runner (high_level_policy/ppo/__init__.py:46-298): ``lrl.ppo.runner.Runner``'s loop —
train rows ``[:num_train_envs]``, eval rows driven by ``act_teacher`` / ``act_student``, ``reset_evaluation_envs`` every
``eval_freq`` iterations, checkpoints every ``save_interval`` and after the loop — over the plain tanh actor-critic.
Video logging is not carried.
"""
import copy
import os

import torch

from ..config import ArgsProto
from ..ppo import runner as _base
from ..ppo.runner import Logger  # noqa: F401
from .actor_critic import ActorCritic
from .ppo import PPO


class RunnerArgs(ArgsProto):
    """__init__.py:46-61"""
    algorithm_class_name = "PPO"
    num_steps_per_env = 200
    max_iterations = 1500
    save_interval = 400
    save_video_interval = 100
    log_freq = 10
    resume = False
    load_run = -1
    checkpoint = -1
    resume_path = None


class Runner(_base.Runner):
    args = RunnerArgs
    actor_critic_class = ActorCritic
    alg_class = PPO

    def _eval_actions(self, obs, priv, hist, n_train, eval_expert):
        ac = self.alg.actor_critic  # (both are actor_body(obs) without a latent)
        if eval_expert:
            return ac.act_teacher(obs[n_train:], priv[n_train:])
        return ac.act_student(obs[n_train:], hist[n_train:])

    def save(self, it):
        """__init__.py:222-235: the state dict as checkpoints/ac_weights_{it:06d}.pt, duplicated to ac_weights_last.pt,
        and the TorchScript actor body as checkpoints/body_latest.jit (nothing without a run directory)."""
        lg = self.logger
        if not lg.run_dir:
            return
        with lg.Sync():
            lg.torch_save(self.alg.actor_critic.state_dict(), f"checkpoints/ac_weights_{it:06d}.pt")
            lg.duplicate(f"checkpoints/ac_weights_{it:06d}.pt", "checkpoints/ac_weights_last.pt")
            body = copy.deepcopy(self.alg.actor_critic.actor_body).to("cpu")
            torch.jit.script(body).save(os.path.join(lg.run_dir, "checkpoints", "body_latest.jit"))
