"""The PPO workspace plans (pure host code: no GPU): lrl_ppo_workspace_bytes, lrl_ppo_act_workspace_bytes and
lrl_ppo_act_student_workspace_bytes against the sizes recorded from the library before the host path was rewritten
around one layer description and one workspace carver (tests/golden/ppo_workspace_bytes.json).  Callers size their
allocations from these calls and tests/test_gemm_multi_gpu.py compares whole workspaces, so no buffer may move.
Regenerate (from a library built at the revision to pin): LRL_LIB=<liblrl.so> python tests/test_ppo_plan.py"""
import ctypes as C
import json
import os

import pytest

from lrl import _abi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_workspace_bytes.json")
ROWS = (37, 200, 256, 24576)
CALLS = ("lrl_ppo_workspace_bytes", "lrl_ppo_act_workspace_bytes", "lrl_ppo_act_student_workspace_bytes")


def _nets():
    from lrl.hlp import ActorCritic as PlainActorCritic
    from lrl.ppo.actor_critic import ActorCritic
    return {"42-obs": ActorCritic(42, 18, 630, 12).flatten_parameters(),
            "235-obs": ActorCritic(235, 18, 3525, 12).flatten_parameters(),
            "plain-14-3": PlainActorCritic(14, 18, 16, 3).flatten_parameters()}


def _sizes(lib):
    out = {}
    for name, net in _nets().items():
        for rows in ROWS:
            row = []
            for call in CALLS:
                f = getattr(lib, call)
                f.restype = C.c_int64
                row.append(int(f(C.byref(net), C.c_int32(rows))))
            out[f"{name}/{rows}"] = row
    return out


def test_workspace_sizes_are_the_recorded_ones():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("liblrl.so not built")
    want = json.load(open(FIXTURE))
    got = _sizes(C.CDLL(_abi.LIB_PATH))
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad
    # the figures the rewrite's issue quotes (update / act / student), and the student call refusing a plain net
    assert want["42-obs/256"] == [14055680, 4849664, 1933312]
    assert want["235-obs/24576"] == [651738112, 242810880, 145178624]
    assert want["plain-14-3/37"] == [1914624, 267776, -1]


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(_sizes(C.CDLL(_abi.LIB_PATH)), f, indent=1)
        f.write("\n")
    print("wrote", FIXTURE)
