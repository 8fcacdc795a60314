#!/usr/bin/env python3
"""The training step from the network's coefficient grid (row A3 of SURVEY.md 8(a)): the plain-torch glue in front of `calc`
(coeffs_grid_to_list -> compute_basis - compute_basis(anchor) -> + pixel positions -> permute, as tests/test_gpu_fullsize.py spells it,
the tile mask moved to the device once) against utils.trajectories_from_grid (one kernel each way, csrc/grid_traj.hip), in ONE process,
A and B alternating: median of 7 blocks of 20 steps after warm-up, host clock ending in a device synchronise.
  node   the grid -> trajectories node alone, forward + backward of a fixed gradient
  step   node + calc + backward to the grid (times drawn on the device every step, as FocusLoss.get_reconstruction_times does)
  loss   calc + backward on precomputed trajectories (the floor the step from the grid is compared with)
Per-kernel times of the fused node from ops.KernelTimer.  Writes profiles/grid_step.json (tagged with build.source_hash()):
    python tools/grid_step_probe.py [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops, utils, build  # noqa: E402
from motionpriorcmax_amd.utils.synth import synth_events  # noqa: E402

BLOCKS, STEPS, WARM = 7, 20, 5
dev = torch.device('cuda:0')


def glue(cg, times, mask, k):
    coeffs, pos, _ = utils.coeffs_grid_to_list(cg, mask, num_coeffs=k)
    traj = utils.compute_basis(coeffs, times, k, 'polynomial') - utils.compute_basis(coeffs, torch.zeros(1, device=dev), k, 'polynomial')
    return (traj + pos[None, :, None, :]).permute(0, 2, 1, 3).contiguous()


def fused(cg, times, mask, k):
    return utils.trajectories_from_grid(cg, times, k, 'polynomial', bench.PATCH)[0]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def main(out):
    res = {'source_hash': build.source_hash(), 'method': f'one process, A/B alternating, median of {BLOCKS} blocks x {STEPS} steps '
           f'after {WARM} warm-up steps; host clock ending in torch.cuda.synchronize(); per-kernel: ops.KernelTimer', 'workloads': {}}
    for name in ('C3', 'C2'):
        wl = bench.WORKLOADS[name]
        B, k = wl['B'], wl['k']
        ev, npos = synth_events(B, wl['M'], (bench.H, bench.W), wl['nb'], seed=1, pad_frac=0.02, time_sorted=True)
        batch = {'events': ev.to(dev), 'num_pos_events': npos}
        L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))
        g = torch.Generator().manual_seed(3)
        cg = (torch.randn(B, 1, 2 * k, bench.H, bench.W, generator=g) * (3.0 if k == 1 else 1.0)).to(dev).requires_grad_(True)
        mask = utils.get_optical_flow_tile_mask((bench.H, bench.W), bench.PATCH).to(dev)       # the reference's registered buffer
        times0 = L.get_reconstruction_times(dev)
        gnode = torch.randn(glue(cg, times0, mask, k).shape, generator=g).to(dev)
        traj_pre = fused(cg, times0, mask, k).detach().clone().requires_grad_(True)

        def node(f):
            def run():
                t = f(cg, L.get_reconstruction_times(dev), mask, k)
                t.backward(gnode)
                cg.grad = None
            return run

        def step(f):
            def run():
                times = L.get_reconstruction_times(dev)
                loss, _, _ = L.calc(f(cg, times, mask, k), times, batch)
                loss.backward()
                cg.grad = None
            return run

        def loss_only():
            loss, _, _ = L.calc(traj_pre, times0, batch)
            loss.backward()
            traj_pre.grad = None

        modes = {'node_glue': node(glue), 'node_fused': node(fused), 'step_glue': step(glue), 'step_fused': step(fused), 'loss_only': loss_only}
        for fn in modes.values():
            for _ in range(WARM):
                fn()
        samples = {m: [] for m in modes}
        for _ in range(BLOCKS):
            for m, fn in modes.items():
                samples[m].append(timed(fn))
        r = {m: {'median_ms': round(statistics.median(v), 4), 'blocks_ms': [round(x, 4) for x in v]} for m, v in samples.items()}
        kern = {}
        for m in ('node_fused', 'step_fused'):
            with ops.KernelTimer() as kt:
                for _ in range(5):
                    modes[m]()
            kern[m] = {kk: {'launches_per_step': v['launches'] / 5, 'avg_us': round(v['avg_us'], 2)}
                       for kk, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
        n = (bench.H // bench.PATCH) * (bench.W // bench.PATCH)
        r['kernels'] = kern
        r['shape'] = dict(grid=[B, 1, 2 * k, bench.H, bench.W], k=k, basis='polynomial', tile=bench.PATCH, n_t=1 + wl['nb'], M=wl['M'])
        r['bytes'] = dict(grad_grid_written=4 * B * 2 * k * bench.H * bench.W, traj_written=8 * B * (1 + wl['nb']) * n,
                          centre_rows_read=4 * B * 2 * k * (bench.H // bench.PATCH) * bench.W, grad_traj_read=8 * B * (1 + wl['nb']) * n)
        res['workloads'][name] = r
        print(name, json.dumps({m: r[m]['median_ms'] for m in modes}), json.dumps(kern['node_fused']), flush=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'grid_step.json'))
