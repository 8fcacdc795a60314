#!/usr/bin/env python3
"""A few eager steps (calc + backward) of one bench.py workload over four rotating batches, with no timers of its own: the command
behind a rocprofv3 run.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/trace_step.py C3 45 [key=value ...]
    python tools/trace_pair_summary.py DIR tag"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from motionpriorcmax_amd import LossFactory
wl = bench.WORKLOADS[sys.argv[1]]
steps = int(sys.argv[2])
over = {}
for kv in sys.argv[3:]:
    k, v = kv.split('='); over[k] = v
dev = torch.device('cuda:0')
sets = []
for j in range(4):
    ev, npos, tr, tm = bench.synth_inputs(wl, seed=1 + 17 * j)
    sets.append(({'events': ev.to(dev), 'num_pos_events': npos}, tr.to(dev).requires_grad_(True)))
tmd = tm.to(dev)
L = LossFactory.get_loss_calculator('FOCUS', dict(bench.loss_config(wl), auto_static_shapes=False, **over))
for i in range(steps):
    b, trd = sets[i % 4]
    loss, _, _ = L.calc(trd, tmd, b)
    loss.backward()
    trd.grad = None
torch.cuda.synchronize()
print('done', sys.argv[1:], flush=True)
