"""The high-level policy's rollout buffer (high_level_policy/ppo/rollout_storage.py): ``lrl.ppo``'s, except that a
minibatch carries no env bins (the reference yields ``None`` there)."""
from ..ppo import rollout_storage as _base


class RolloutStorage(_base.RolloutStorage):
    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        for batch in super().mini_batch_generator(num_mini_batches, num_epochs):
            yield batch[:-1] + (None,)
