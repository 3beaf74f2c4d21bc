"""``from mini_gym_learn.eval_metrics.domain_randomization import DR_SETTINGS, base_set``: the reference's evaluation
presets, called as there (``base_set(); DR_SETTINGS["static_low"]()`` edit the module-level ``Cfg`` in place).

The settings themselves are this project's table ``lrl.config.EVAL_PRESETS`` (cfg path -> value); each function applies
one entry of it.  ``static_low`` keeps the reference's ``motor_strength_range = [0.9, -0.99]`` (see the table).  For an
eval group beside a training cfg use ``lrl.config.eval_variant(cfg, n, sets, preset=NAME)`` (scripts/train.py
--eval-preset) with one of the DR presets; ``base_set`` changes per-step kernel parameters and suits a stand-alone
evaluation env only (scripts/evaluate.py)."""
from lrl import config as _config
from mini_gym.envs.base.legged_robot_config import Cfg


def _setter(name):
    def apply():
        _config._apply(Cfg, _config.EVAL_PRESETS[name])
    apply.__name__ = apply.__qualname__ = name
    apply.__doc__ = f"Set the {name!r} entries of lrl.config.EVAL_PRESETS on Cfg."
    return apply


base_set = _setter("base_set")
DR_SETTINGS = {name: _setter(name) for name in _config.DR_PRESETS}
globals().update(DR_SETTINGS)  # rand_regular(), static_low(), ... by name, as the reference's module has them
