"""Evaluation metrics and presets on the host: the float64 checker (tests/metrics_ref.py) and the torch forms of
``mini_gym_learn.eval_metrics.metrics.METRICS_FNS`` against the reference's recorded outputs
(tests/golden/eval_metrics.npz), the preset table against what the reference's functions assign
(tests/golden/dr_settings.json), the presets through eval_variant -> eval_group_params, and the ABI additions.  No GPU."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import metrics_ref
from helpers import GOLDEN, ROBOT_FILES, golden
from lrl import _abi
from lrl import config as lcfg
from lrl import params as lparams
from lrl.robot import load_robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("base_lin_vel", "base_ang_vel", "commands", "torques", "dof_vel", "root_states", "payloads", "reset_buf")


@pytest.fixture(scope="module")
def fx():
    return golden("eval_metrics.npz")


@pytest.fixture(scope="module")
def dr_fixture():
    with open(os.path.join(GOLDEN, "dr_settings.json")) as f:
        return json.load(f)


def _inputs(fx, prefix):
    return {k: fx[prefix + k] for k in INPUTS + ("measured_heights",)}


def _ref(fx, prefix, heights):
    a = _inputs(fx, prefix)
    h = a.pop("measured_heights")
    return metrics_ref.metrics(default_body_mass=float(fx["default_body_mass"]), measured_heights=h if heights else 0, **a)


# ---- 1. the checker reproduces the reference
@pytest.mark.parametrize("form", ["h", "s"], ids=["heights_7x187", "heights_scalar_0"])
def test_checker_reproduces_the_reference(fx, form):
    ref = _ref(fx, "in_", form == "h")
    got = {k: fx[f"{form}_{k}"] for k in metrics_ref.NAMES}
    assert all(got[k].shape == (7,) for k in got)
    assert np.isfinite(got["CoT"]).all()
    worst = metrics_ref.check(got, ref, rows=metrics_ref.NAMES, what=form)
    print({k: round(v, 4) for k, v in worst.items()})  # the reference's float32 error in units of each bar


def test_zero_speed_cot_is_not_finite(fx):
    ref = _ref(fx, "zero_in_", True)
    assert not np.isfinite(ref["CoT"]).any() and not np.isfinite(fx["zero_CoT"]).any()
    metrics_ref.check({k: fx["zero_" + k] for k in metrics_ref.NAMES}, ref, rows=metrics_ref.NAMES, what="zero speed")


def test_metric_names_and_abi_rows(fx):
    assert tuple(fx["numeric"]) == metrics_ref.NAMES == _abi.METRIC_NAMES
    assert metrics_ref.ROWS[_abi.METRIC_SPEED_XY] == "speed_xy" and len(metrics_ref.ROWS) == _abi.METRIC_ROWS


# ---- 2. METRICS_FNS / DR_SETTINGS / base_set against the fixtures
def _namespace_env(fx, prefix, heights):
    env = types.SimpleNamespace(**{k: torch.from_numpy(v) for k, v in _inputs(fx, prefix).items()})
    env.default_body_mass = float(fx["default_body_mass"])
    if not heights:
        env.measured_heights = 0
    return env


def test_metrics_fns_keys_and_signature(fx):
    import inspect

    from mini_gym_learn.eval_metrics.metrics import METRICS_FNS
    assert list(METRICS_FNS) == list(fx["names"])
    for name, fn in METRICS_FNS.items():
        assert list(inspect.signature(fn).parameters) == ["env", "actor_critic", "obs"], name
        assert fn.__name__ == name


@pytest.mark.parametrize("form", ["h", "s", "zero"])
def test_metrics_fns_torch_forms_reproduce_the_reference(fx, form):
    from mini_gym_learn.eval_metrics.metrics import METRICS_FNS
    prefix = "zero_in_" if form == "zero" else "in_"
    env = _namespace_env(fx, prefix, form != "s")
    ref = _ref(fx, prefix, form != "s")
    b = metrics_ref.bars(ref)
    for name in metrics_ref.NAMES:
        out = METRICS_FNS[name](env, None, None)
        assert isinstance(out, torch.Tensor) and out.device.type == "cpu", name
        want = fx[f"{form}_{name}"]
        assert out.dtype == torch.from_numpy(want).dtype and tuple(out.shape) == want.shape, name
        got, fin = out.numpy().astype(np.float64), np.isfinite(want)
        assert not np.isfinite(got[~fin]).any(), name
        # both are float32 evaluations of the same expression: each within the bar of the float64 value
        assert np.all(np.abs(got[fin] - want[fin].astype(np.float64)) <= 2 * b[name][fin]), name
    assert not np.isfinite(fx["zero_CoT"]).any()


def test_network_metrics_and_auxiliary_rewards(fx):
    from mini_gym_learn.eval_metrics.metrics import METRICS_FNS
    A, B = torch.from_numpy(fx["net_A"]), torch.from_numpy(fx["net_B"])
    ac = types.SimpleNamespace(adaptation_module=lambda h: h @ A, env_factor_encoder=lambda p: torch.tanh(p @ B))
    obs = {"obs_history": torch.from_numpy(fx["obs_history"]), "privileged_obs": torch.from_numpy(fx["privileged_obs_in"])}
    env = _namespace_env(fx, "in_", True)
    r = [torch.from_numpy(fx["aux_r0"]), torch.from_numpy(fx["aux_r1"])]
    env.reward_functions, env.reward_names, env.reward_scales = [lambda: r[0], lambda: r[1]], ["a", "b"], {"a": 2.0, "b": 3.0}
    al = METRICS_FNS["adaptation_loss"](env, ac, obs)
    assert isinstance(al, torch.Tensor) and al.device.type == "cpu"
    np.testing.assert_allclose(al.numpy(), fx["h_adaptation_loss"], rtol=1e-6, atol=1e-7)
    assert METRICS_FNS["adaptation_loss"](env, types.SimpleNamespace(), obs) is None  # no adaptation module
    po, lat = METRICS_FNS["privileged_obs"](env, ac, obs), METRICS_FNS["latents"](env, ac, obs)
    assert isinstance(po, np.ndarray) and isinstance(lat, np.ndarray)
    assert np.array_equal(po, fx["h_privileged_obs"])
    np.testing.assert_allclose(lat, fx["h_latents"], rtol=1e-6, atol=1e-7)
    aux = METRICS_FNS["auxiliary_rewards"](env, ac, obs)
    assert list(aux) == list(fx["h_aux_names"]) == ["a"]  # the first term only, as the reference returns
    np.testing.assert_allclose(aux["a"].numpy(), fx["h_auxiliary_rewards_a"], rtol=1e-7)


def test_preset_table_equals_what_the_reference_assigns(dr_fixture):
    assert set(dr_fixture) == set(lcfg.EVAL_PRESETS) and set(lcfg.DR_PRESETS) == set(dr_fixture) - {"base_set"}
    for name, want in dr_fixture.items():
        have = lcfg.EVAL_PRESETS[name]
        assert set(have) == set(want), name
        for path in want:
            assert have[path] == want[path] and type(have[path]) is type(want[path]), (name, path)
    assert lcfg.EVAL_PRESETS["static_low"]["domain_rand.motor_strength_range"] == [0.9, -0.99]  # the reference's value


def _flat(d, prefix=""):
    """A cfg dict as {dotted path: leaf}; dict-valued fields (gains, joint angles) are leaves."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict) and k not in ("stiffness", "damping", "default_joint_angles"):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


def test_dr_settings_and_base_set_edit_cfg_as_the_reference(dr_fixture):
    import copy

    from mini_gym.envs.base.legged_robot_config import Cfg
    from mini_gym_learn.eval_metrics import domain_randomization as dr
    assert list(dr.DR_SETTINGS) == ["rand_regular", "rand_large", "static_low", "static_medium", "static_high",
                                    "only_base_mass"]
    saved = copy.deepcopy(Cfg)
    try:
        for name, fn in dict(dr.DR_SETTINGS, base_set=dr.base_set).items():
            assert getattr(dr, name) is fn
            Cfg.__dict__.clear()
            Cfg.__dict__.update(copy.deepcopy(saved).__dict__)
            before = Cfg.to_dict()
            fn()
            after = Cfg.to_dict()
            fb, fa = _flat(before), _flat(after)
            # (by repr: tests that ran before may have left arrays in the shared Cfg)
            changed = {k: v for k, v in fa.items() if k not in fb or repr(fb[k]) != repr(v)}
            want = dr_fixture[name]
            assert set(changed) <= set(want), (name, set(changed) - set(want))  # nothing else moved
            for path, v in want.items():
                assert fa[path] == v, (name, path)
    finally:
        Cfg.__dict__.clear()
        Cfg.__dict__.update(saved.__dict__)


# ---- 3. every preset as an eval cfg
@pytest.fixture(scope="module")
def rob():
    return load_robot(ROBOT_FILES["mc"])


def _mc_cfg():
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.terrain.x_offset = 0
    return cfg


@pytest.mark.parametrize("name", ["rand_regular", "rand_large", "static_low", "static_medium", "static_high",
                                  "only_base_mass"])
def test_dr_presets_are_valid_eval_cfgs(rob, name, dr_fixture):
    cfg = _mc_cfg()
    ev = lcfg.eval_variant(cfg, 25, preset=name)
    assert ev.env.num_envs == 25 and cfg.env.num_envs != 25
    for path, v in dr_fixture[name].items():
        node = ev
        for p in path.split("."):
            node = getattr(node, p)
        assert node == v, path
    G = lparams.eval_group_params(lparams.build_params(cfg, rob), lparams.build_params(ev, rob))  # no NotImplementedError
    lo, hi = dr_fixture[name]["domain_rand.motor_strength_range"]
    if [lo, hi] != list(cfg.domain_rand.motor_strength_range):
        assert isinstance(G, _abi.LrlGroupParams)
        assert [np.float32(x) for x in G.motor_strength_range] == [np.float32(lo), np.float32(hi)]
        assert np.float32(G.dr_span[0]) == np.float32(hi - lo)
    # an explicit set comes after the preset; the --eval-set strings of a preset give the same cfg
    ev2 = lcfg.eval_variant(cfg, 25, ["domain_rand.friction_range=[0.2,0.3]"], preset=name)
    assert ev2.domain_rand.friction_range == [0.2, 0.3]
    assert lcfg.eval_variant(cfg, 25, lcfg.preset_sets(name)).to_dict() == ev.to_dict()


def test_base_set_and_terminal_body_height_stay_refused(rob):
    cfg = _mc_cfg()
    P = lparams.build_params(cfg, rob)
    with pytest.raises(NotImplementedError, match="terminal_body_height"):
        lparams.eval_group_params(P, lparams.build_params(
            lcfg.eval_variant(cfg, 8, ["rewards.terminal_body_height=0.05"], preset="static_medium"), rob))
    with pytest.raises(NotImplementedError, match="max_episode_length"):
        lparams.eval_group_params(P, lparams.build_params(lcfg.eval_variant(cfg, 8, preset="base_set"), rob))
    both = lcfg.eval_variant(cfg, 8, preset=("base_set", "static_high"))  # a stand-alone evaluation env's cfg
    assert both.env.episode_length_s == 500 and both.domain_rand.friction_range == [4.49, 4.5]
    with pytest.raises(KeyError, match="static_hgih"):
        lcfg.eval_variant(cfg, 8, preset="static_hgih")


def test_runner_args_default_off():
    from lrl.ppo.runner import RunnerArgs
    assert RunnerArgs.log_eval_metrics is False


# ---- 4. ABI
def test_new_symbols_resolve_and_abi_version_stays():
    L = _abi.lib()
    assert L.lrl_abi_version() == 6
    for name in ("lrl_sim_metrics_enable", "lrl_sim_metrics_clear", "lrl_sim_metrics_tensors", "lrl_sim_metrics_reduce"):
        assert getattr(L, name).restype is C.c_int32
    null = C.c_void_p()
    for call in (lambda: L.lrl_sim_metrics_enable(null, C.c_int32(1)), lambda: L.lrl_sim_metrics_clear(null, null),
                 lambda: L.lrl_sim_metrics_tensors(null, None),  # (lrl_metrics_view* out: a null struct pointer)
                 lambda: L.lrl_sim_metrics_reduce(null, C.c_int32(0), C.c_int32(0), null, null)):
        assert call() == -1  # LRL_E_INVALID on a null sim: no launch


def test_metric_ids_and_view_layout_match_header(tmp_path):
    import subprocess
    names = [f for f, _ in _abi.LrlMetricsView._fields_]
    ids = ["LRL_METRIC_" + k.upper() for k in _abi.METRIC_NAMES] + ["LRL_METRIC_NUM", "LRL_METRIC_SPEED_XY",
                                                                   "LRL_METRIC_ROWS", "LRL_METRICS_REDUCE_DOUBLES"]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "lrl.h"\nint main(){\n' \
           'printf("%zu\\n", sizeof(lrl_metrics_view));\n' + \
           "".join(f'printf("%zu\\n", offsetof(lrl_metrics_view, {f}));\n' for f in names) + \
           "".join(f'printf("%d\\n", (int){i});\n' for i in ids) + "return 0;}\n"
    exe = str(tmp_path / "lrl_metrics_layout")
    with open(exe + ".c", "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, exe + ".c"])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    n = _abi.METRIC_NUM
    assert out == [C.sizeof(_abi.LrlMetricsView)] + [getattr(_abi.LrlMetricsView, f).offset for f in names] + \
        list(range(n)) + [n, _abi.METRIC_SPEED_XY, _abi.METRIC_ROWS, _abi.METRICS_REDUCE_DOUBLES]
