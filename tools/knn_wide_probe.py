#!/usr/bin/env python3
"""The chunked KNN route (n >= 65536 trajectories per sample: ops.knn_wide_fwd, csrc/knn_wide.hip) timed on the shapes of bench.py:
C2 and C3 with `patch_size` 2 (n = 240 x 320 = 76 800, two chunks) and, beside them for scale, the same workloads at the shipped
patch_size 4 (n = 19 200, the native route).  Per shape: ms per eager `calc` + backward step (host clock around a device synchronise,
median of three windows), microseconds per step of every kernel (mpc_profile_start / mpc_profile_stop: HIP events around every
launch, in a pass of its own) and the peak of torch's allocated memory.  Writes profiles/knn_wide.json.

    python tools/knn_wide_probe.py [--steps 10] [--out profiles/knn_wide.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops, utils  # noqa: E402
from motionpriorcmax_amd.build import source_hash  # noqa: E402
from motionpriorcmax_amd.utils.synth import bin_mid_times  # noqa: E402


def trajectories(wl, patch, seed):
    """bench.synth_inputs' polynomial trajectories with the tile size as a parameter (config key `patch_size` of the reference)."""
    g = torch.Generator().manual_seed(seed + 7)
    k = wl['k']
    times = torch.cat((torch.tensor([0.41]), bin_mid_times(wl['nb'])))
    mask = utils.get_optical_flow_tile_mask((bench.H, bench.W), patch)
    coeff = torch.randn(wl['B'], 1, 2 * k, bench.H, bench.W, generator=g) * (3.0 if k == 1 else 1.0)
    coeffs, pos, _ = utils.coeffs_grid_to_list(coeff, mask, num_coeffs=k)
    traj = utils.compute_basis(coeffs, times, k, 'polynomial') - utils.compute_basis(coeffs, torch.zeros(1), k, 'polynomial')
    return (traj + pos[None, :, None, :]).permute(0, 2, 1, 3).contiguous(), times


def probe(name, patch, steps, dev):
    wl = bench.WORKLOADS[name]
    ev, npos, _, _ = bench.synth_inputs(wl, seed=1)
    tr, tm = trajectories(wl, patch, seed=1)
    L = LossFactory.get_loss_calculator('FOCUS', dict(bench.loss_config(wl), auto_static_shapes=False))
    batch = {'events': ev.to(dev), 'num_pos_events': npos}
    trd, tmd = tr.to(dev).requires_grad_(True), tm.to(dev)

    def step():
        loss, _, _ = L.calc(trd, tmd, batch)
        loss.backward()
        trd.grad = None
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    for _ in range(3):
        step()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / steps)
    peak = torch.cuda.max_memory_allocated(dev)
    with ops.KernelTimer() as kt:
        for _ in range(steps):
            step()
    kernels = {k: round(v['total_us'] / steps, 1) for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
    n = tr.shape[2]
    out = dict(workload=name, patch_size=patch, n=n, route='chunked' if ops.knn_is_wide(n) else 'native',
               chunks=len(ops.knn_chunk_starts(n, bench.KNN)) - 1 if ops.knn_is_wide(n) else 1, B=wl['B'], events=wl['M'], num_bins=wl['nb'],
               step_ms=round(1e3 * sorted(ts)[1], 4), step_ms_windows=[round(1e3 * t, 4) for t in ts], steps_per_window=steps,
               peak_allocated_mb=round(peak / 2 ** 20, 1), inputs_allocated_mb=round(base / 2 ** 20, 1), kernel_us_per_step=kernels)
    print(f"{name} patch {patch} n={n} {out['route']:8s} {out['step_ms']:.3f} ms/step  peak {out['peak_allocated_mb']} MB  "
          + ' '.join(f'{k}={v}' for k, v in list(kernels.items())[:6]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_wide.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = [probe(name, patch, args.steps, dev) for name in ('C2', 'C3') for patch in (2, 4)]
    doc = dict(tool='tools/knn_wide_probe.py', device=torch.cuda.get_device_name(dev), source_hash=source_hash(), shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
