"""The rollout act's two paths over the row count: the one-launch act (LRL_ACT_FUSED=1) against the GEMM chain
(LRL_ACT_FUSED=0), the preset network, HIP events around K calls of each (alternated in blocks, the median block
reported).  The table sets ACT_FUSED_MAX_ROWS (csrc/lrl_ppo.hip).  usage: python scripts/act_rows.py [K] [rows ...]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rapid-locomotion-rl_amd"))
import torch  # noqa: E402

from lrl.ppo.actor_critic import ActorCritic  # noqa: E402
from lrl.ppo.rollout_storage import RolloutStorage  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROWS = [int(x) for x in sys.argv[2:]] or [1024, 4096, 16384, 65536]
BLOCKS = 5
ac = ActorCritic(42, 18, 630, 12).cuda()
print(f"{'rows':>7s} {'one launch us':>14s} {'chain us':>10s} {'ratio':>6s}")
for n in ROWS:
    st = RolloutStorage(n, 4, [42], [18], [630], [12], "cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(0)
    obs, priv, hist = (torch.randn(n, k, device="cuda:0", generator=g) for k in (42, 18, 630))
    desc = st.store_desc()
    t = {"1": [], "0": []}
    for b in range(BLOCKS + 1):  # (block 0: warm-up)
        for fused in ("1", "0"):
            os.environ["LRL_ACT_FUSED"] = fused
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for i in range(K):
                ac.act_fused(obs, priv, hist, seed=1, counter=i + 1, store=desc, store_row=i % 4)
            ev1.record()
            torch.cuda.synchronize()
            if b:
                t[fused].append(ev0.elapsed_time(ev1) / K * 1e3)
    one, chain = statistics.median(t["1"]), statistics.median(t["0"])
    print(f"{n:7d} {one:14.1f} {chain:10.1f} {one / chain:6.2f}")
