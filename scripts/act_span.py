"""The rollout act in a rocprofv3 --kernel-trace CSV of bench.py: per rollout step, the span from the end of
extras_snapshot_kernel to the start of the next shift_history_kernel (the act's wall time on the stream) and the summed
duration and count of the kernels launched inside it.  Means over those of the last TAIL steps that show the most common launch pattern (env TAIL, default 120: bench.py's
5 timed iterations x 24 steps).  usage: python scripts/act_span.py <kernel_trace.csv>"""
import csv
import os
import sys
from collections import Counter

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
spans = []
i = 0
while i < len(rows):
    if "extras_snapshot_kernel" in rows[i][2]:
        j = i + 1
        while j < len(rows) and "shift_history_kernel" not in rows[j][2] and "extras_snapshot_kernel" not in rows[j][2]:
            j += 1
        if j < len(rows) and "shift_history_kernel" in rows[j][2]:
            inside = rows[i + 1:j]
            spans.append((rows[j][0] - rows[i][1], sum(e - s for s, e, _ in inside), len(inside),
                          tuple(n.split("(")[0][-60:] for _, _, n in inside)))
        i = j
    else:
        i += 1
tail = spans[-int(os.environ.get("TAIL", "120")):]
assert tail, "no extras_snapshot_kernel -> shift_history_kernel pair in the trace"
# the steps of the most common launch pattern (the rare others span an iteration boundary: the update's launches)
names, c = Counter(s[3] for s in tail).most_common(1)[0]
tail = [s for s in tail if s[3] == names]
n = len(tail)
print(f"steps {n}: span {sum(s[0] for s in tail) / n / 1e3:.1f} us, kernels inside {sum(s[1] for s in tail) / n / 1e3:.1f} us "
      f"in {len(names)} launches")
print("  " + " | ".join(names))
