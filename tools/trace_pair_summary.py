#!/usr/bin/env python3
"""Per-step figures from the kernel trace of `rocprofv3 --kernel-trace -- python3 tools/trace_step.py ...`: step period, every kernel's
duration and the gap behind it (median [min .. max] over the warm steps, us), and contrast + smoothness as one figure: the fused
launch, or the two launches plus the launch boundary behind k_lut_smooth_march.
    python tools/trace_pair_summary.py DIR tag"""
import csv, glob, statistics as st, sys
d, tag = sys.argv[1], sys.argv[2]
f = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)[0]
rows = sorted(([r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])] for r in csv.DictReader(open(f))), key=lambda r: r[1])
def short(n): return n.split('(')[0].split('<')[0].replace('void ', '').strip()
rows = [[short(n), a, b] for n, a, b in rows]
# a step starts at k_knn_bucket (first kernel of the forward)
first = rows[0][0]
starts = [i for i, r in enumerate(rows) if r[0] == 'k_knn_bucket']
if not starts: print(tag, 'no k_knn_bucket; first kernel', first); sys.exit(0)
steps = [rows[a:b] for a, b in zip(starts, starts[1:])]
steps = steps[len(steps) // 3:]            # warm steps only
def med(v): return st.median(v) / 1e3
def rng(v): return f'{med(v):7.2f} [{min(v)/1e3:6.2f} .. {max(v)/1e3:6.2f}]'
period = [b[0][1] - a[0][1] for a, b in zip(steps, steps[1:])]
busy = [sum(r[2] - r[1] for r in s) for s in steps]
span = [s[-1][2] - s[0][1] for s in steps]
print(f'{tag}: {len(steps)} steps, {len(steps[0])} launches per step; period us {rng(period)}  span {rng(span)}  sum of kernels {rng(busy)}')
names = ['k_contrast_smooth_march', 'k_contrast_march', 'k_lut_smooth_march']
pair = []
for s in steps:
    tot = 0
    for i, r in enumerate(s):
        if r[0] in names:
            tot += r[2] - r[1]
            if r[0] == 'k_lut_smooth_march' and i + 1 < len(s): tot += s[i + 1][1] - r[2]      # the launch boundary behind it
    pair.append(tot)
print(f'{tag}: contrast + smoothness (+ one launch boundary where they are two launches) us {rng(pair)}')
per = {}
for s in steps:
    for i, r in enumerate(s):
        per.setdefault(r[0], []).append(r[2] - r[1])
        if i + 1 < len(s): per.setdefault('gap after ' + r[0], []).append(s[i + 1][1] - r[2])
for k, v in per.items():
    if not k.startswith('gap'): print(f'   {k:32s} {rng(v)}   gap behind {rng(per.get("gap after " + k, [0]))}')
