"""Per position of one graph replay: the kernel and its mean duration over the timed steps of
the common length (a step ends with its second ccc_finish_kernel).
usage: python scripts/step_positions.py run_results.db 200  (a rocprofv3 --kernel-trace rocpd database of
`bench.py --full --steps 200`; profiles/group16/step_kernels*.txt)"""
import sqlite3
import sys
from collections import Counter

db, steps = sys.argv[1], int(sys.argv[2])
c = sqlite3.connect(db)
rows = c.execute("select name, start, end, duration from kernels order by start").fetchall()
first_probe = next((i for i, r in enumerate(rows) if "noop_kernel" in r[0]), len(rows))
timed = rows[:first_probe]
finish = [i for i, r in enumerate(timed) if "ccc_finish_kernel" in r[0]]
ends = finish[1::2][-steps - 1:]          # the last kernel index of each of the last steps + 1
per = [timed[a + 1:b + 1] for a, b in zip(ends[:-1], ends[1:])]
n = Counter(len(p) for p in per).most_common(1)[0][0]
use = [p for p in per if len(p) == n]
print(f"{len(per)} steps, {len(use)} of {n} dispatches (lengths {dict(Counter(len(p) for p in per))})")
tot = 0.0
for i in range(n):
    names = Counter(p[i][0] for p in use)
    nm = names.most_common(1)[0][0]
    ds = [p[i][3] for p in use if p[i][0] == nm]
    avg = sum(ds) / len(ds) / 1e3
    tot += avg
    if "gemm" in nm:
        short = nm.replace("_ZN3jmt", "").replace("void jmt::", "")[:64]
        print(f"{i:3d} {avg:8.2f} us  {short}")
print(f"sum of mean kernel durations {tot / 1e3:.4f} ms/step")
