"""The ``__main__`` flow of the reference's scripts/high_level_play.py on this framework: load a trained low-level
(locomotion) policy, build the navigation env over it (``HighLevelControlWrapper`` with 1,024 envs), and train the
high-level policy with ``high_level_policy.ppo.Runner(env).learn(1000, eval_freq=200, eval_expert=True)``.

The low-level checkpoint is an argument: a ``.pt`` state dict of ``mini_gym_learn.ppo.ActorCritic`` (35 keys, e.g. a
run's ``checkpoints/ac_weights_last.pt``) or an ``.npz`` holding the same tensors as ``sd/<key>`` with their names in
``keys`` (the layout of tests/golden/checkpoint_last.npz).

``--timing K`` runs K iterations after one warm-up iteration and prints one JSON line: ms per iteration, split into
the rollout (200 wrapper steps, each a low-level policy act and env step plus the wrapper's torch) and the update,
and the update's share of the split-bf16 MFMA bound of its GEMM FLOPs.  ``--fused 0`` trains with the torch-autograd
update instead of the native one (the comparison the timing is for).  ``--native 1`` runs the wrapper's own step on
the device (``HighLevelControlWrapper(native=True)``: six launches per step and no host read, in place of the wrapper's
torch); the default is the host-torch wrapper.

usage: python scripts/high_level_train.py LOW_LEVEL_CHECKPOINT [--iterations N] [--num-envs N] [--steps T]
                                          [--robot go1|mc] [--root DIR] [--fused 0|1] [--native 0|1] [--timing K]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rapid-locomotion-rl_amd"))

X6_PEAK_TF = 2500.0 / 6  # dense bf16 MFMA peak over the six products of an fp32 product (bench.py)


def load_low_level(path):
    import numpy as np
    import torch
    from mini_gym_learn.ppo import ActorCritic
    if path.endswith(".npz"):
        g = np.load(path, allow_pickle=False)
        sd = {str(k): torch.from_numpy(g["sd/" + str(k)]) for k in g["keys"]}
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    ac = ActorCritic(42, 18, 630, 12)
    ac.load_state_dict(sd, strict=True)
    return ac


def update_gemm_flops(runner):
    """fp32 FLOPs of one update's GEMMs: forward, backward-data (layers 2 and 3) and weight gradient of the three
    [actor; critic] layer pairs over every minibatch row of every epoch (the heads and Adam are not products)."""
    from high_level_policy.ppo.ppo import PPO_Args
    ac = runner.alg.actor_critic
    dims = [ac.num_obs] + [m.out_features for m in ac.actor_body if hasattr(m, "out_features")][:3]
    per_row = 0
    for i, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        per_row += 2 * 2 * k * n * (3 if i else 2)  # actor + critic; forward, dW (+ dX past the first layer)
    s = runner.alg.storage
    rows = (s.num_envs * s.num_transitions_per_env) // PPO_Args.num_mini_batches * PPO_Args.num_mini_batches
    return per_row * rows * PPO_Args.num_learning_epochs


def timed_learn(runner, iters, eval_freq, eval_expert):
    """One warm-up iteration, then ``iters`` timed ones: (ms per iteration, ms of it in the update), device-synchronised."""
    import torch
    upd = runner.alg.update
    spent = [0.0]

    def timed_update():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = upd()
        torch.cuda.synchronize()
        spent[0] += time.perf_counter() - t0
        return out

    runner.alg.update = timed_update
    runner.learn(1, eval_freq=eval_freq, eval_expert=eval_expert)
    torch.cuda.synchronize()
    spent[0] = 0.0
    t0 = time.perf_counter()
    runner.learn(iters, eval_freq=eval_freq, eval_expert=eval_expert)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    runner.alg.update = upd
    return 1e3 * total / iters, 1e3 * spent[0] / iters


if __name__ == "__main__":
    from pathlib import Path

    ap = argparse.ArgumentParser()
    ap.add_argument("low_level", help="low-level policy checkpoint (.pt state dict or .npz)")
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=None, help="RunnerArgs.num_steps_per_env (default 200)")
    ap.add_argument("--robot", default="go1", choices=["go1", "mc"])
    ap.add_argument("--root", default=None, help="run root (default: <package>/high_level_policy/runs)")
    ap.add_argument("--fused", type=int, default=1, choices=[0, 1], help="0: the torch-autograd update")
    ap.add_argument("--native", type=int, default=0, choices=[0, 1], help="1: the wrapper's step on the device")
    ap.add_argument("--timing", type=int, default=0, help="time this many iterations and print one JSON line")
    a = ap.parse_args()

    from high_level_policy import HLP_ROOT_DIR
    from high_level_policy.ppo import Runner, RunnerArgs
    from lrl.high_level import HighLevelControlWrapper
    from ml_logger import logger

    env = HighLevelControlWrapper.from_actor_critic(load_low_level(a.low_level), num_envs=a.num_envs, device="cuda:0",
                                                    robot=a.robot, native=bool(a.native))
    stem = Path(__file__).stem
    logger.configure(logger.utcnow(f"rapid-locomotion/%Y-%m-%d/{stem}/%H%M%S.%f"),
                     root=Path(a.root or f"{HLP_ROOT_DIR}/high_level_policy/runs").resolve())
    logger.log_text("""
                charts:
                - yKey: train/episode/rew_total/mean
                  xKey: iterations
                """, filename=".charts.yml", dedent=True)
    if a.steps is not None:
        RunnerArgs.num_steps_per_env = a.steps
    runner = Runner(env, device="cuda:0", fused=bool(a.fused))
    if a.timing:
        ms_iter, ms_update = timed_learn(runner, a.timing, eval_freq=200, eval_expert=True)
        flops = update_gemm_flops(runner)
        print(json.dumps(dict(workload=f"{a.num_envs} envs x {runner.num_steps_per_env} steps", fused=bool(a.fused),
                              native=bool(a.native),
                              iterations=a.timing, ms_per_iteration=round(ms_iter, 2),
                              ms_rollout=round(ms_iter - ms_update, 2), ms_update=round(ms_update, 2),
                              update_gemm_gflop=round(flops / 1e9, 2),
                              update_share_of_x6_bound=round(flops / (X6_PEAK_TF * 1e12) / (ms_update * 1e-3), 4))))
    else:
        runner.learn(num_learning_iterations=a.iterations, eval_freq=200, eval_expert=True)
