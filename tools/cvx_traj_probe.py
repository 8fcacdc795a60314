#!/usr/bin/env python3
"""The RAFT-spline output head -> trajectories node (utils.trajectories_from_bezier(..., up_mask=...) -> ops.CvxCurveTrajFn,
csrc/cvx_curves.hip) against its plain-torch mirror (utils/basis.py: softmax, pad, nine shifted multiply-adds, gather at the tile
centres, einsum) on the same GPU in ONE process, A and B alternating: median of 7 blocks of 10 steps after warm-up, host clock ending
in a device synchronise.  bench.py's C4 and C4b6 workloads: 480 x 640 (h x w = 60 x 80), d = 10, n_t = 42, tile 4, B = 1 and B = 6.
  node   forward + backward of a fixed gradient to params and up_mask
  step   node + FocusLoss.calc + backward to params and up_mask
Per-kernel times of the fused node from ops.KernelTimer, and the bandwidth they amount to over the bytes the algorithm needs
(computed from the shapes below).  Writes profiles/cvx_traj.json (tagged with build.source_hash()):
    python tools/cvx_traj_probe.py [out.json]"""
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
from motionpriorcmax_amd.utils import basis as ub  # noqa: E402
from motionpriorcmax_amd.utils.synth import synth_events  # noqa: E402

BLOCKS, STEPS, WARM = 7, 10, 3
H, W, TILE = bench.H, bench.W, bench.PATCH
D, NB = bench.WORKLOADS['C4']['k'], bench.WORKLOADS['C4']['nb']
dev = torch.device('cuda:0')


def fused(p, m, times):
    return utils.trajectories_from_bezier(p, times, TILE, (H, W), up_mask=m)[0]


def mirror(p, m, times):
    bm = ub._device_basis('bernstein', times, (D,), p.device, p.dtype)
    _, pos_dev = ub._tile_positions(H, W, TILE, p.device, p.dtype)
    return ub._cvx_curve_trajectories_mirror(p, m, bm, pos_dev, 1.0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def algorithmic_bytes(B):
    h, w = H // 8, W // 8
    n, n_t = (H // TILE) * (W // TILE), 1 + NB
    params, chans, traj = 4 * B * 2 * D * h * w, 4 * B * 9 * (8 // TILE) ** 2 * h * w, 8 * B * n_t * n
    return dict(forward=params + chans + traj, backward=traj + chans + params + params + 4 * B * 576 * h * w,
                params=params, mask_channels_touched=chans, traj=traj, grad_mask=4 * B * 576 * h * w)


def main(out):
    res = {'source_hash': build.source_hash(), 'method': f'one process, A/B alternating, median of {BLOCKS} blocks x {STEPS} steps after '
           f'{WARM} warm-up steps; host clock ending in torch.cuda.synchronize(); per-kernel: ops.KernelTimer',
           'shape': dict(image=[H, W], d=D, n_t=1 + NB, tile=TILE), 'batches': {}}
    for name in ('C4', 'C4b6'):
        wl = bench.WORKLOADS[name]
        B, M = wl['B'], wl['M']
        L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))
        g = torch.Generator().manual_seed(3)
        p = (torch.randn(B, 2 * D, H // 8, W // 8, generator=g) * 0.5).to(dev).requires_grad_(True)
        m = (torch.randn(B, 576, H // 8, W // 8, generator=g) * 2.0).to(dev).requires_grad_(True)
        ev, npos = synth_events(B, M, (H, W), NB, seed=1, pad_frac=0.02, time_sorted=True)
        batch = {'events': ev.to(dev), 'num_pos_events': npos}
        times = L.get_reconstruction_times(dev)
        gnode = torch.randn(B, 1 + NB, (H // TILE) * (W // TILE), 2, generator=g).to(dev)

        def clear():
            p.grad = m.grad = None

        def node(f):
            def run():
                f(p, m, times).backward(gnode)
                clear()
            return run

        def step(f):
            def run():
                loss, _, _ = L.calc(f(p, m, times), times, batch)
                loss.backward()
                clear()
            return run

        def fwd_only():
            with torch.no_grad():
                fused(p, m, times)

        modes = {'node_mirror': node(mirror), 'node_fused': node(fused), 'step_mirror': step(mirror), 'step_fused': step(fused),
                 'forward_fused': fwd_only}
        for fn in modes.values():
            for _ in range(WARM):
                fn()
        samples = {k: [] for k in modes}
        for _ in range(BLOCKS):
            for k, fn in modes.items():
                samples[k].append(timed(fn))
        r = {k: {'median_ms': round(statistics.median(v), 4), 'blocks_ms': [round(x, 4) for x in v]} for k, v in samples.items()}
        with ops.KernelTimer() as kt:
            for _ in range(5):
                modes['node_fused']()
        kern = {k: {'launches_per_step': v['launches'] / 5, 'avg_us': round(v['avg_us'], 2)}
                for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
        by = algorithmic_bytes(B)
        fwd_us = sum(v['avg_us'] for k, v in kern.items() if 'fwd' in k)
        bwd_us = sum(v['avg_us'] for k, v in kern.items() if 'bwd' in k)
        r['kernels'] = kern
        r['fused_forward_us'], r['fused_backward_us'] = round(fwd_us, 2), round(bwd_us, 2)
        r['bytes'] = by
        r['workload'] = dict(name=name, B=B, events_per_sample=M)
        r['achieved_GBps'] = dict(forward=round(by['forward'] / fwd_us / 1e3, 1), backward=round(by['backward'] / bwd_us / 1e3, 1))
        r['fused_faster_than_mirror'] = bool(r['node_fused']['median_ms'] < r['node_mirror']['median_ms'] and
                                             r['step_fused']['median_ms'] < r['step_mirror']['median_ms'])
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps({k: r[k]['median_ms'] for k in modes}), json.dumps(kern), json.dumps(r['achieved_GBps']), flush=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'cvx_traj.json'))
