"""Per position of one graph replay: the kernel and its mean duration over the timed steps, from
a rocprofv3 --kernel-trace CSV of a bench.py run (profiles/tail/step_kernels*.txt).  A step ends
with the second CCC finish of the step: ccc_finish_kernel, or ccc_stats_finish_kernel where the
statistics and the finish are one launch.  Prints every position, then the head / tail kernels'
totals.
usage: python scripts/tail_positions.py kernel_trace.csv [steps]"""
import csv
import sys
from collections import Counter

path = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
rows = []
with open(path, newline="") as f:
    for r in csv.DictReader(f):
        rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
rows.sort(key=lambda r: r[1])
first_probe = next((i for i, r in enumerate(rows) if "noop_kernel" in r[0]), len(rows))
timed = rows[:first_probe]
is_finish = lambda n: "ccc_finish_kernel" in n or "ccc_stats_finish_kernel" in n
finish = [i for i, r in enumerate(timed) if is_finish(r[0])]
ends = finish[1::2][-steps - 1:]
per = [timed[a + 1:b + 1] for a, b in zip(ends[:-1], ends[1:])]
n = Counter(len(p) for p in per).most_common(1)[0][0]
use = [p for p in per if len(p) == n]
print(f"{len(per)} steps, {len(use)} of {n} dispatches (lengths {dict(Counter(len(p) for p in per))})")


def short(nm):
    nm = nm.replace("void jmt::", "").replace("jmt::", "")
    return nm.split("(")[0][:72]


tot = 0.0
fam = Counter()
for i in range(n):
    nm = Counter(p[i][0] for p in use).most_common(1)[0][0]
    ds = [p[i][2] - p[i][1] for p in use if p[i][0] == nm]
    avg = sum(ds) / len(ds) / 1e3
    tot += avg
    print(f"{i:3d} {avg:8.2f} us  {short(nm)}")
    for key in ("head_fwd_kernel", "head_bwd_kernel", "head_reduce_kernel", "copy2d_kernel",
                "copy_rows_vec_kernel", "ccc_stats_kernel", "ccc_finish_kernel",
                "ccc_stats_finish_kernel", "ccc_bwd_kernel"):
        if key in nm:
            fam[key] += avg
span = [(p[-1][2] - p[0][1]) / 1e3 for p in use]
print(f"sum of mean kernel durations {tot / 1e3:.4f} ms/step; mean first-start-to-last-end "
      f"{sum(span) / len(span) / 1e3:.4f} ms")
for key, v in sorted(fam.items()):
    print(f"  {key:28s} {v:8.2f} us/step")
