"""The folded backward tail inside the training step, from a rocprofv3 --kernel-trace csv of bench.py:
python tools/tail_trace.py <kernel_trace.csv>
For every step (k_forward, k_backward, the tail's launches up to k_fold_finish): the launches between them (median us each), the tail's span
(k_backward's end -> k_fold_finish's end), its kernel time and the boundaries (span - kernels), and the step period
(k_forward start -> next k_forward start) where the steps run back to back inside a graph."""
import csv
import re
import statistics
import sys


def short(name):
    m = re.search(r"\bk_[a-z0-9_]+", name)
    return m.group(0) if m else name


rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]))
               for r in csv.DictReader(open(sys.argv[1]))), key=lambda r: r[0])
per, spans, kern, periods = {}, [], [], []
last_fwd = None
for i, (t0, t1, k) in enumerate(rows[:-2]):
    # a step: k_forward, then k_backward right behind it, then the tail up to k_fold_finish (the spin-up's and the
    # per-kernel timing's isolated launches repeat one kernel back to back and are not steps)
    if k != "k_forward" or rows[i + 1][2] != "k_backward" or rows[i + 1][0] - t1 > 20_000:
        continue
    b1 = rows[i + 1][1]
    tail = []
    for u0, u1, kk in rows[i + 2:i + 7]:
        tail.append((u0, u1, kk))
        if kk == "k_fold_finish":
            break
    if not tail or tail[-1][2] != "k_fold_finish" or tail[-1][1] - b1 > 100_000:
        continue
    if last_fwd is not None and t0 - last_fwd < 250_000:
        periods.append((t0 - last_fwd) / 1e3)
    last_fwd = t0
    for u0, u1, kk in tail:
        per.setdefault(kk, []).append((u1 - u0) / 1e3)
    spans.append((tail[-1][1] - b1) / 1e3)
    kern.append(sum(u1 - u0 for u0, u1, _ in tail) / 1e3)

med = statistics.median
print(f"steps with a folded tail: {len(spans)}")
for k, v in per.items():
    print(f"  {k:16s} median {med(v):6.2f} us  (min {min(v):6.2f}, max {max(v):6.2f}, n {len(v)})")
print(f"  tail kernels     median {med(kern):6.2f} us")
print(f"  tail span        median {med(spans):6.2f} us  (k_backward end -> k_fold_finish end)")
print(f"  boundaries       median {med([s - k for s, k in zip(spans, kern)]):6.2f} us")
if periods:
    print(f"step period (k_forward -> k_forward of consecutive steps): median {med(periods):6.2f} us, n {len(periods)}")
