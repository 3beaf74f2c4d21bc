"""The rollout step between two env kernels in a rocprofv3 --kernel-trace CSV of bench.py: per step, the span from
the end of one env_step_kernel to the start of the next (everything a rollout step does besides the physics: extras
snapshot, storage row, act, history shift) and the summed duration and count of the kernels launched inside it.  Means
over those of the last TAIL steps that show the most common launch pattern (env TAIL, default 120: bench.py's 5 timed
iterations x 24 steps; the rare others span an iteration boundary, the update's launches).  Also counts, over the whole
trace and over the window of those TAIL steps, the launches of the two kernels a rollout step can do without
(act_span.py is anchored on them and finds nothing once they are gone).
usage: python scripts/step_span.py <kernel_trace.csv>"""
import csv
import os
import sys
from collections import Counter

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
short = lambda n: n.split("(")[0][-60:]
env = [i for i, r in enumerate(rows) if "env_step_kernel" in r[2]]
spans = []
for a, b in zip(env, env[1:]):
    inside = rows[a + 1:b]
    spans.append((rows[b][0] - rows[a][1], sum(e - s for s, e, _ in inside), len(inside),
                  tuple(short(n) for _, _, n in inside), rows[a][1], rows[b][0]))
tail = spans[-int(os.environ.get("TAIL", "120")):]
assert tail, "fewer than two env_step_kernel launches in the trace"
t0, t1 = tail[0][4], tail[-1][5]
names, c = Counter(s[3] for s in tail).most_common(1)[0]
steps = [s for s in tail if s[3] == names]
n = len(steps)
print(f"steps {n} of the last {len(tail)}: span {sum(s[0] for s in steps) / n / 1e3:.1f} us, kernels inside "
      f"{sum(s[1] for s in steps) / n / 1e3:.1f} us in {len(names)} launches, idle {sum(s[0] - s[1] for s in steps) / n / 1e3:.1f} us")
print("  " + " | ".join(names))
for k in ("extras_snapshot_kernel", "shift_history_kernel"):
    whole = sum(k in r[2] for r in rows)
    window = sum(k in r[2] and t0 <= r[0] <= t1 for r in rows)
    print(f"{k}: {whole} launches in the trace, {window} in the window of the last {len(tail)} steps")
