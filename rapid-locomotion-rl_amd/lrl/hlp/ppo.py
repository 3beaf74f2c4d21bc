"""PPO for the high-level policy (high_level_policy/ppo/ppo.py with USE_LATENT = False).

``lrl.ppo.ppo.PPO`` with the high-level policy's own argument class, and without what the plain network lacks: no
adaptation-module regression (``update`` returns 0 for its loss, as the reference does), no second stream, and no
``infos['env_bins']`` (the reference's ``process_env_step`` does not read it; the wrapper's infos carry none).
"""
import torch

from ..config import ArgsProto
from ..ppo import ppo as _base
from .actor_critic import ActorCritic
from .rollout_storage import RolloutStorage


class PPO_Args(ArgsProto):
    """ppo.py:17-32"""
    value_loss_coef = 1.0
    use_clipped_value_loss = True
    clip_param = 0.2
    entropy_coef = 0.01
    num_learning_epochs = 5
    num_mini_batches = 4
    learning_rate = 1.e-3
    adaptation_module_learning_rate = 1.e-3
    num_adaptation_module_substeps = 1
    schedule = "adaptive"
    gamma = 0.99
    lam = 0.95
    desired_kl = 0.01
    max_grad_norm = 1.


class PPO(_base.PPO):
    actor_critic: ActorCritic
    args = PPO_Args
    storage_class = RolloutStorage

    def __init__(self, actor_critic, device="cpu", fused=None, seed=0):
        super().__init__(actor_critic, device=device, fused=fused, seed=seed)
        self.overlap_adaptation = False  # there is no adaptation chain to overlap
        self._no_bins = None

    def process_env_step(self, rewards, dones, infos):
        if "env_bins" not in infos:  # the storage's env_bins row stays zero (the reference stores none)
            if self._no_bins is None or self._no_bins.shape != rewards.shape or self._no_bins.device != rewards.device:
                self._no_bins = torch.zeros_like(rewards, dtype=torch.float32)
            infos = dict(infos, env_bins=self._no_bins)
        super().process_env_step(rewards, dones, infos)

    def _adaptation_substeps(self, hist_b, priv_b, params):
        return torch.zeros((), device=self.device)
