#!/usr/bin/env python3
"""Alternate two builds of the library (build_ab/libmpcmax_parent.so, build_ab/libmpcmax_new.so, loaded through MPC_AB_LIB) over
`bench.py --workload W`, N pairs per workload; ms_per_step of every run, then median / min / max per build.  Stops at the first
failing run.
    python tools/ab_bench_series.py out.txt 6 C3,C2,C4"""
import json, os, subprocess, sys
out = sys.argv[1]; pairs = int(sys.argv[2]); wls = sys.argv[3].split(',')
res = {}
with open(out, 'a') as f:
    for wl in wls:
        for i in range(pairs):
            for tag, lib in (('parent', 'build_ab/libmpcmax_parent.so'), ('new', 'build_ab/libmpcmax_new.so')):
                env = dict(os.environ, MPC_AB_LIB=lib)
                p = subprocess.run(['timeout', '-k', '10', '150', sys.executable, 'bench.py', '--workload', wl], env=env, capture_output=True, text=True)
                if p.returncode != 0:
                    print('FAILED', wl, tag, p.returncode, p.stderr[-2000:]); sys.exit(p.returncode)
                ms = json.loads(p.stdout.strip().splitlines()[-1])['ms_per_step']
                res.setdefault((wl, tag), []).append(ms)
                line = f'{wl} pair {i} {tag} {ms:.4f}'
                print(line, flush=True); f.write(line + '\n'); f.flush()
    for (wl, tag), v in res.items():
        s = sorted(v); med = (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2
        line = f'SUMMARY {wl} {tag} median {med:.4f} min {s[0]:.4f} max {s[-1]:.4f} runs {v}'
        print(line, flush=True); f.write(line + '\n')
