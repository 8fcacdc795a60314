#!/usr/bin/env python3
"""Step and per-kernel times of FocusLoss.calc_per_event_curves with a tabulated curve basis that TRAINS, at the C4 shapes of
tools/pe_curves_probe.py (480 x 640, 1 x 500 k and 6 x 500 k events, 41 bins, sp = 4, d = 10, S = 1024, control points on the 1/8
grid with their convex-upsampling mask), on a time-sorted batch (the loader's) and on a bucket-ordered one:

    trainable    the fused node (ops.PerEventCurvesFn) with basis_table.requires_grad: mpc_pec_table_basis_grad + mpc_pec_field_basis_grad
                 beside the step of a constant table, phim built in the graph
    frozen       the same step with the table a constant (what the node ran before a table could train)
    plain_torch  fused=False with the trainable table: phi [B, M, 10] in the graph around the vote / objective kernels

Median of `--steps` steps per route (forward + backward), the routes ALTERNATING inside every round of one process, every step
timed from the host with a device synchronisation on both sides; then the per-kernel times of 3 steps from ops.KernelTimer, with
k_pec_table_grad's time beside the passes of the row gradient (k_pec_accum on bucket-ordered rows, k_pec_grad_atomic otherwise)
of the same step.  The table is a random walk (a smooth basis, as a trained one is); all three routes see the same tensors.

--frozen-lines NAME=FILE,...: outputs of `tools/pe_curves_probe.py --curve TABLE --routes fused` (the frozen-table step) taken on
the parent commit and on this one in one session, alternating; their medians go into the JSON as they are.

    python tools/pec_table_probe.py [--out FILE] [--steps 15] [--workloads C4,C4b6] [--routes trainable,frozen,plain_torch]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops  # noqa: E402
from motionpriorcmax_amd.build import source_hash  # noqa: E402
from motionpriorcmax_amd.utils.synth import synth_events  # noqa: E402

TABLE_SAMPLES = 1024
ROWS_GRAD_KERNELS = ('k_pec_accum', 'k_pec_grad_atomic')


def frozen_lines(spec):
    """{name: {workload: {layout: {median_ms, min_ms, p90_ms}}}} of pe_curves_probe outputs (route `fused`, curve TABLE)."""
    out = {}
    for item in spec.split(','):
        name, path = item.split('=', 1)
        r = json.load(open(path))
        out[name] = {'source_hash': r.get('source_hash'), 'workloads': {
            w: {ln: {k: lv['fused'][k] for k in ('median_ms', 'min_ms', 'p90_ms', 'library_kernels_total_us')} for ln, lv in wv['layouts'].items()}
            for w, wv in r['workloads'].items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pec_table.json'))
    ap.add_argument('--routes', default='trainable,frozen,plain_torch')
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--workloads', default='C4,C4b6')
    ap.add_argument('--frozen-lines', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'steps': args.steps, 'source_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'table_samples': TABLE_SAMPLES,
              'workloads': {}}
    if args.frozen_lines:
        result['frozen_step_pe_curves_probe_curve_TABLE'] = frozen_lines(args.frozen_lines)
    for wname in args.workloads.split(','):
        wl = bench.WORKLOADS[wname]
        B, d, nb = wl['B'], wl['k'], wl['nb']
        H, W = bench.H, bench.W
        ev, npos = synth_events(B, wl['M'], (H, W), nb, seed=1, pad_frac=0.02, time_sorted=True)
        L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))
        g = torch.Generator().manual_seed(8)
        params = (torch.randn(B, 2 * d, H // 8, W // 8, generator=g) * 0.25).to(dev).requires_grad_(True)      # (x 8 in the upsampling: N(0, 2^2) pixels)
        mask = torch.randn(B, 576, H // 8, W // 8, generator=g).to(dev).requires_grad_(True)
        walk = torch.cumsum(torch.randn(TABLE_SAMPLES + 1, d, generator=g) * (0.5 / math.sqrt(TABLE_SAMPLES)), 0)
        table = walk.to(dev).requires_grad_(True)
        frozen = walk.to(dev)
        t_ref = torch.full((1,), 0.41, device=dev)
        sorted_b = {'events': ev.to(dev), 'num_pos_events': npos}
        batches = {'time_sorted': sorted_b, 'bucket_ordered': L.order_events(sorted_b)}
        out_w = {'desc': wl['desc'] + '; control points on the 1/8 grid + up_mask; TABLE, S = 1024', 'sp': bench.SP, 'd': d, 'layouts': {}}

        def clear():
            params.grad = None
            mask.grad = None
            table.grad = None

        for lname, b in batches.items():
            def r_trainable():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, curve_type='TABLE', basis_table=table)[0].backward()

            def r_frozen():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, curve_type='TABLE', basis_table=frozen)[0].backward()

            def r_plain_torch():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, curve_type='TABLE', basis_table=table, fused=False)[0].backward()
            every = {'trainable': r_trainable, 'frozen': r_frozen, 'plain_torch': r_plain_torch}
            routes = {n: every[n] for n in args.routes.split(',')}
            times_ms = {n: [] for n in routes}
            for fn in routes.values():
                for _ in range(2):
                    fn()
                    clear()
            torch.cuda.synchronize()
            for _ in range(args.steps):
                for n, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times_ms[n].append(1e3 * (time.perf_counter() - t0))
                    clear()
            out = {}
            for n, fn in routes.items():
                with ops.KernelTimer() as kt:
                    for _ in range(3):
                        fn()
                        clear()
                ks = {kn: round(v['total_us'] / 3, 1) for kn, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
                ts = sorted(times_ms[n])
                out[n] = {'median_ms': round(statistics.median(ts), 4), 'min_ms': round(ts[0], 4), 'p90_ms': round(ts[int(0.9 * (len(ts) - 1))], 4),
                          'library_kernels_us_per_step': ks, 'library_kernels_total_us': round(sum(ks.values()), 1)}
                if n == 'trainable':
                    out[n]['table_pass_beside_the_row_gradient_us'] = {
                        'k_pec_table_grad': ks.get('k_pec_table_grad'),
                        'row_gradient_passes': {kn: v for kn, v in ks.items() if kn.startswith(ROWS_GRAD_KERNELS)}}
                print(f'{wname} {lname} {n}: median {out[n]["median_ms"]} ms (min {out[n]["min_ms"]}, p90 {out[n]["p90_ms"]}); library kernels '
                      f'{out[n]["library_kernels_total_us"]} us: ' + ' '.join(f'{a}={v}' for a, v in list(ks.items())[:9]), flush=True)
            out_w['layouts'][lname] = out
        result['workloads'][wname] = out_w
        del batches, sorted_b, params, mask, table, frozen
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
