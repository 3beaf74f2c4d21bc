"""The high-level policy's actor-critic (high_level_policy/ppo/actor_critic.py with USE_LATENT = False).

Only ``actor_body``, ``critic_body`` and ``std``: 17 state-dict keys.  Both bodies read the observations alone; the
privileged observations and the observation history that the reference's call signatures carry are accepted and
ignored.  ``flatten_parameters`` describes the network to the native calls as a plain net (``lrl_ppo_net.plain = 1``)
with the module's activation.
"""
import torch
import torch.nn as nn

from .. import _abi
from ..config import ArgsProto
from ..ppo import actor_critic as _base
from ..ppo.actor_critic import get_activation  # noqa: F401


class AC_Args(ArgsProto):
    """actor_critic.py:10-21 (the encoder / adaptation entries are carried for the reference's surface, unused)"""
    init_noise_std = 1.0
    actor_hidden_dims = [512, 256, 128]
    critic_hidden_dims = [512, 256, 128]
    activation = "tanh"
    adaptation_module_branch_hidden_dims = [[256, 32]]
    env_factor_encoder_branch_input_dims = [18]
    env_factor_encoder_branch_latent_dims = [18]
    env_factor_encoder_branch_hidden_dims = [[256, 128]]


_ACTIVATION_CODE = {nn.ELU: 0, nn.Tanh: 1}  # lrl_ppo_net.activation


class ActorCritic(_base.ActorCritic):
    def __init__(self, num_obs, num_privileged_obs, num_obs_history, num_actions, **kwargs):
        nn.Module.__init__(self)
        act = get_activation(AC_Args.activation)
        self.actor_body = _base._mlp([num_obs] + AC_Args.actor_hidden_dims + [num_actions], act)
        self.critic_body = _base._mlp([num_obs] + AC_Args.critic_hidden_dims + [1], act)
        self.std = nn.Parameter(AC_Args.init_noise_std * torch.ones(num_actions))
        self.num_obs, self.num_privileged_obs, self.num_actions = num_obs, num_privileged_obs, num_actions
        self.num_obs_history = num_obs_history
        self.distribution = None

    def update_distribution(self, observations, privileged_observations=None):
        mean = self.actor_body(observations)
        self.distribution = torch.distributions.Normal(mean, mean * 0.0 + self.std, validate_args=False)

    def act_inference(self, ob, policy_info={}):
        return self.act_student(ob["obs"], ob["obs_history"])

    def act_student(self, observations, observation_history=None, policy_info={}):
        return self.actor_body(observations)

    def act_teacher(self, observations, privileged_info=None, policy_info={}):
        return self.actor_body(observations)

    def evaluate(self, critic_observations, privileged_observations=None, **kwargs):
        return self.critic_body(critic_observations)

    def act_student_fused(self, obs, hist=None):
        raise RuntimeError("the high-level policy has no adaptation module: act_student is actor_body(obs)")

    def flatten_parameters(self):
        """As the base's, for the plain form: [actor; critic] layer pairs, the heads, ``std``, one KL slot; no encoder
        and no adaptation region (``adapt_begin == adapt_end``)."""
        net = getattr(self, "_net", None)
        if net is not None and self.std.data_ptr() == self._flat.data_ptr() + 4 * net.std_off:
            return net
        A = [m for m in self.actor_body if isinstance(m, nn.Linear)]
        Cb = [m for m in self.critic_body if isinstance(m, nn.Linear)]
        if len(A) != 4 or len(Cb) != 4:
            raise ValueError("lrl_ppo expects 4-layer actor/critic MLPs")
        code = _ACTIVATION_CODE.get(type(self.actor_body[1]))
        if code is None:
            raise ValueError("lrl_ppo implements the ELU and tanh activations only")
        if A[0].in_features != self.num_obs or [m.out_features for m in Cb[:3]] != [m.out_features for m in A[:3]]:
            raise ValueError("actor and critic must share hidden sizes and take the observations alone")
        net = _abi.LrlPpoNet()
        order, off = [], 0

        def put(name, *tensors, align=64):
            nonlocal off
            off = (off + align - 1) // align * align
            setattr(net, name, off)
            for t in tensors:
                order.append((t, off))
                off += t.numel()

        net.main_begin = 0
        for i, nm in enumerate(("1", "2", "3")):
            put("w" + nm, A[i].weight, Cb[i].weight)
            put("b" + nm, A[i].bias, Cb[i].bias)
        put("w4a", A[3].weight); put("b4a", A[3].bias); put("w4c", Cb[3].weight); put("b4c", Cb[3].bias)
        put("std_off", self.std)
        net.main_end = net.kl_slot = off
        off = (off + 1 + 63) // 64 * 64
        net.adapt_begin = net.adapt_end = off
        net.total = off
        flat = torch.zeros(net.total, device=self.std.device)
        with torch.no_grad():
            for t, o in order:
                flat[o:o + t.numel()].copy_(t.detach().reshape(-1))
            for t, o in order:
                t.data = flat[o:o + t.numel()].view_as(t)
        net.num_obs, net.num_priv = self.num_obs, self.num_privileged_obs
        net.num_hist, net.num_actions = self.num_obs_history, self.num_actions
        net.ac_h0, net.ac_h1, net.ac_h2 = A[0].out_features, A[1].out_features, A[2].out_features
        net.activation, net.plain = code, 1
        self._flat, self._net = flat, net
        return net
