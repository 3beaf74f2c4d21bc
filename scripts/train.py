"""The reference's scripts/train.py flow (scripts/train.py:1-54) on this framework: the same imports — isaacgym and
ml_logger resolve to the package's stand-ins — and the same calls (logger.configure / log_text / log_params,
VelocityTrackingEasyEnv, HistoryWrapper, Runner(env, device), runner.learn).  The reference's own file runs unchanged
against the package too (tests/test_script_surface.py checks what it imports and calls); this copy only adds
--iterations / --robot / --root so a short run can be asked for, and --terrain-tgs (the project-only key
Cfg.sim.physx.terrain_solver_type = 1: a terrain mesh then solves contacts with the presets' TGS, as the reference's
PhysX does, instead of this project's default PGS there; no effect on the plane), and --eval-envs / --eval-set: an
eval group of N envs after the train envs (the reference's eval_cfg), driven by the student policy and logged under
eval/episode, whose cfg is a copy of the train cfg with every PATH=VALUE applied (VALUE a python literal).  The eval
cfg may differ in command ranges and in domain randomisation, pushes and teleport; e.g. a narrow
low-friction evaluation without pushes:
  --eval-envs 512 --eval-set domain_rand.friction_range=[0.05,0.06] --eval-set domain_rand.push_robots=False
--eval-preset NAME is sugar over --eval-set: one of the reference's evaluation DR presets (lrl.config.DR_PRESETS:
rand_regular, rand_large, static_low, static_medium, static_high, only_base_mass), applied before the explicit sets.
usage: python scripts/train.py [--iterations N] [--robot mc|go1] [--root DIR] [--terrain-tgs]
                               [--eval-envs N [--eval-preset NAME] [--eval-set PATH=VALUE ...]]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))


def train_mc(headless=True, iterations=4000, robot="go1", terrain_tgs=False, eval_envs=0, eval_set=()):
    import isaacgym
    assert isaacgym
    import torch  # noqa: F401

    from mini_gym.envs.base.legged_robot_config import Cfg
    from mini_gym.envs.go1.go1_config import config_go1
    from mini_gym.envs.mini_cheetah.mini_cheetah_config import config_mini_cheetah
    from mini_gym.envs.mini_cheetah.velocity_tracking import VelocityTrackingEasyEnv
    from mini_gym.envs.wrappers.history_wrapper import HistoryWrapper
    from mini_gym_learn.ppo import Runner, RunnerArgs
    from mini_gym_learn.ppo.actor_critic import AC_Args
    from mini_gym_learn.ppo.ppo import PPO_Args
    from ml_logger import logger

    (config_mini_cheetah if robot == "mc" else config_go1)(Cfg)  # (the reference's file: config_go1)
    if terrain_tgs:
        Cfg.sim.physx.terrain_solver_type = 1
    eval_cfg = None
    if eval_envs:
        from lrl.config import eval_variant
        eval_cfg = eval_variant(Cfg, eval_envs, eval_set)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=headless, cfg=Cfg, eval_cfg=eval_cfg)
    logger.log_params(AC_Args=vars(AC_Args), PPO_Args=vars(PPO_Args), RunnerArgs=vars(RunnerArgs), Cfg=vars(Cfg))
    env = HistoryWrapper(env)
    runner = Runner(env, device="cuda:0")
    runner.learn(num_learning_iterations=iterations, init_at_random_ep_len=True, eval_freq=100)
    return runner


if __name__ == "__main__":
    from pathlib import Path

    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4000)
    ap.add_argument("--robot", default="go1", choices=["mc", "go1"])
    ap.add_argument("--root", default=None, help="run root (default: <package>/runs, as MINI_GYM_ROOT_DIR/runs)")
    ap.add_argument("--terrain-tgs", action="store_true",
                    help="on a terrain mesh follow Cfg.sim.physx.solver_type (TGS in the presets) instead of PGS")
    ap.add_argument("--eval-envs", type=int, default=0, help="envs of an eval group after the train envs (0: none)")
    ap.add_argument("--eval-set", action="append", default=[], metavar="PATH=VALUE",
                    help="set a field of the eval cfg (a copy of the train cfg), e.g. "
                         "domain_rand.friction_range=[0.05,0.06]; repeatable")
    from lrl.config import DR_PRESETS, preset_sets
    ap.add_argument("--eval-preset", default=None, choices=list(DR_PRESETS), metavar="NAME",
                    help="an evaluation DR preset for the eval cfg (%s), set before the --eval-set items"
                         % ", ".join(DR_PRESETS))
    a = ap.parse_args()
    if (a.eval_set or a.eval_preset) and not a.eval_envs:
        ap.error("--eval-set / --eval-preset need --eval-envs")
    if a.eval_preset:
        a.eval_set = preset_sets(a.eval_preset) + a.eval_set
    from ml_logger import logger
    from mini_gym import MINI_GYM_ROOT_DIR

    stem = Path(__file__).stem
    logger.configure(logger.utcnow(f"rapid-locomotion/%Y-%m-%d/{stem}/%H%M%S.%f"),
                     root=Path(a.root or f"{MINI_GYM_ROOT_DIR}/runs").resolve())
    logger.log_text("""
                charts:
                - yKey: train/episode/rew_total/mean
                  xKey: iterations
                - yKey: train/episode/command_area/mean
                  xKey: iterations
                """, filename=".charts.yml", dedent=True)
    train_mc(headless=True, iterations=a.iterations, robot=a.robot, terrain_tgs=a.terrain_tgs,
             eval_envs=a.eval_envs, eval_set=a.eval_set)
