"""``from mini_gym_learn.eval_metrics.metrics import METRICS_FNS``: the reference's per-step evaluation metrics, same
names and ``(env, actor_critic, obs)`` signature, each returning a CPU tensor (numpy for privileged_obs / latents).

For a native env (``lrl.env.LeggedRobotEnv``, also behind wrappers) the state metrics are rows of the device table the
metrics kernel writes in every step (``lrl.eval_metrics.EvalMetrics``; enabled on first use): the values of the step's
post-physics state, before that step's resets.  Until the first step after enabling, and for any other object, they are
the plain torch expressions over the env's attributes.  Code that wants statistics rather than per-step copies should
use ``EvalMetrics.summary`` instead: these functions keep the reference's one copy per metric and step."""
import torch

from lrl.eval_metrics import GRAVITY, EvalMetrics

FROUDE_LEG_LENGTH = 0.30


def _native(env):
    while not hasattr(env, "_sim") and hasattr(env, "env"):
        env = env.env
    return env if hasattr(env, "_sim") else None


def _row(env, name):
    """The table row of a native env once a step has written it, else None."""
    e = _native(env)
    if e is None:
        return None
    m = getattr(e, "_metrics_fns", None)
    if m is None:
        m = e._metrics_fns = EvalMetrics(e)
    if not m.enabled:
        m.enable()
        m.enabled_at = e.common_step_counter
    if e.common_step_counter <= getattr(m, "enabled_at", -1):
        return None
    return m.step_values()[name].cpu()


def _power(env):
    return torch.sum(env.torques * env.dof_vel, dim=1)


# the torch forms: name -> f(env) on the env's device
_TORCH = {
    "lin_vel_rmsd": lambda env: torch.sqrt(torch.square(env.base_lin_vel[:, 0] - env.commands[:, 0])),
    "ang_vel_rmsd": lambda env: torch.sqrt(torch.square(env.base_ang_vel[:, 2] - env.commands[:, 2])),
    "lin_vel_x": lambda env: env.base_lin_vel[:, 0],
    "ang_vel_yaw": lambda env: env.base_ang_vel[:, 2],
    # measured_heights is the scalar 0 on an env without a height scan: the mean is then root z
    "base_height": lambda env: (env.root_states[:, 2:3] - env.measured_heights).mean(dim=1),
    "max_torques": lambda env: env.torques.abs().amax(dim=1),
    "power_consumption": _power,
    # P / (m g |v_xy|): inf / nan for a robot that stands still
    "CoT": lambda env: _power(env) / ((env.default_body_mass + env.payloads) * GRAVITY
                                      * torch.linalg.vector_norm(env.base_lin_vel[:, :2], dim=1)),
    "froude_number": lambda env: torch.square(env.base_lin_vel[:, 0]) / (GRAVITY * FROUDE_LEG_LENGTH),
}


def _state_metric(name):
    def fn(env, actor_critic, obs):
        row = _row(env, name)
        return row if row is not None else _TORCH[name](env).detach().cpu()
    fn.__name__ = fn.__qualname__ = name
    return fn


lin_vel_rmsd = _state_metric("lin_vel_rmsd")
ang_vel_rmsd = _state_metric("ang_vel_rmsd")
lin_vel_x = _state_metric("lin_vel_x")
ang_vel_yaw = _state_metric("ang_vel_yaw")
base_height = _state_metric("base_height")
max_torques = _state_metric("max_torques")
power_consumption = _state_metric("power_consumption")
CoT = _state_metric("CoT")
froude_number = _state_metric("froude_number")


def adaptation_loss(env, actor_critic, obs):
    """Per-env mean squared error of the adaptation module against the encoder's latent (None without the module)."""
    if not hasattr(actor_critic, "adaptation_module"):
        return None
    with torch.no_grad():
        pred = actor_critic.adaptation_module(obs["obs_history"]).cpu()
        target = actor_critic.env_factor_encoder(obs["privileged_obs"]).cpu()
    return torch.square(pred - target).mean(dim=1)


def auxiliary_rewards(env, actor_critic, obs):
    # The reference returns from inside its loop over the reward terms, so the dict holds the first term only (None
    # for an env without terms); that observable behaviour is kept, not the every-term dict the name suggests.
    for name, fn in zip(env.reward_names, env.reward_functions):
        return {name: (fn() * env.reward_scales[name]).detach().cpu()}
    return None


def termination(env, actor_critic, obs):
    """The reset flags (bool, as env.reset_buf): a native env's are those of the last step either way."""
    return env.reset_buf.detach().cpu()


def privileged_obs(env, actor_critic, obs):
    return obs["privileged_obs"].detach().cpu().numpy()


def latents(env, actor_critic, obs):
    with torch.no_grad():
        return actor_critic.env_factor_encoder(obs["privileged_obs"]).cpu().numpy()


METRICS_FNS = {fn.__name__: fn for fn in (
    lin_vel_rmsd, ang_vel_rmsd, lin_vel_x, ang_vel_yaw, base_height, max_torques, power_consumption, CoT,
    froude_number, adaptation_loss, auxiliary_rewards, termination, privileged_obs, latents)}
