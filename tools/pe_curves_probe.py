#!/usr/bin/env python3
"""Step and per-kernel times of the per-event continuous-time warp along RAFT-spline curves (FocusLoss.calc_per_event_curves) at
bench.py's C4 and C4-batch-6 shapes (480 x 640, 500 k events per sample, 41 bins, sp = 4, Bezier degree 10, control points on the
1/8 grid with their convex-upsampling mask), on a time-sorted batch (the loader's) and on a bucket-ordered one, beside the two
routes a caller could already run:

    fused      the new node (ops.PerEventCurvesFn, csrc/pe_curves.hip): basis in registers
    unfused    (a) calc_per_event_curves(fused=False): rows and phi [B, M, 10] in plain torch around the generic per-event kernels
    lut        (b) trajectories_from_bezier(up_mask=) + calc: 41 time bins, the KNN look-up table, time constant per bin

Median of `--steps` steps per route (forward + backward), the routes ALTERNATING inside every round of one process, every step
timed from the host with a device synchronisation on both sides; then the per-kernel times of 3 steps from ops.KernelTimer, and
the passes of the ordered row gradient (mpc_pec_rows_grad_passes).

--curve BEZIER (the default) is the above, written to profiles/pe_curves.json.  --curve BSPLINE and --curve TABLE time the cubic
B-spline of 11 control points instead, written to profiles/pe_curves_bspline.json: `fused` is the named kind -- 'BSPLINE', exact and
in registers, or 'TABLE', the same basis sampled at S = 1024 (bspline_basis) and interpolated --, `fused_other` the other of the two
in the same alternation, `lut` trajectories_from_curves(curve_type='BSPLINE') + calc; `unfused` only with --routes.  With a
B-spline kind the bucket-ordered layout also times k_pec_accum at 1 and 3 orders per pass beside the library's choice.

    python tools/pe_curves_probe.py [--curve BEZIER] [--out FILE] [--steps 15] [--workloads C4,C4b6] [--routes fused,lut]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops, utils, _lib as C  # noqa: E402
from motionpriorcmax_amd.build import source_hash  # noqa: E402
from motionpriorcmax_amd.utils.synth import synth_events, bin_mid_times  # noqa: E402


TABLE_SAMPLES = 1024


class _OrdersPerPass:
    """ops.PerEventCurvesFn with `orders_per_pass` fixed (FocusLoss.calc_per_event_curves always takes the library's choice)."""

    def __init__(self, fn, k):
        self.fn, self.k = fn, k

    def apply(self, *a):
        return self.fn.apply(*a, self.k)


def orders_per_pass_sweep(sh, d, step, clear, rounds=5):
    """k_pec_accum per step (us, median of `rounds` alternating rounds) at the library's choice (0), 1 and 3 orders per pass."""
    real = ops.PerEventCurvesFn
    got = {k: [] for k in (0, 1, 3)}
    try:
        for _ in range(rounds):
            for k in got:
                ops.PerEventCurvesFn = _OrdersPerPass(real, k)
                with ops.KernelTimer() as kt:
                    step()
                    clear()
                got[k].append(sum(v['total_us'] for n, v in kt.summary().items() if n.startswith('k_pec_accum')))          # (k_pec_accum_bsp)
    finally:
        ops.PerEventCurvesFn = real
    return {str(k): {'median_us': round(statistics.median(v), 1), 'min_us': round(min(v), 1), 'max_us': round(max(v), 1),
                     'passes': int(C.lib().mpc_pec_rows_grad_passes(ctypes.byref(sh), d, k))} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--curve', choices=('BEZIER', 'BSPLINE', 'TABLE'), default='BEZIER')
    ap.add_argument('--out', default=None)
    ap.add_argument('--routes', default=None, help='comma list out of fused, fused_other, unfused, lut (default: all of the curve)')
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--workloads', default='C4,C4b6')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'pe_curves.json' if args.curve == 'BEZIER' else 'pe_curves_bspline.json')
    dev = torch.device('cuda:0')
    result = {'steps': args.steps, 'source_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'workloads': {}}
    for wname in args.workloads.split(','):
        wl = bench.WORKLOADS[wname]
        B, d, nb = wl['B'], wl['k'], wl['nb']
        H, W = bench.H, bench.W
        ev, npos = synth_events(B, wl['M'], (H, W), nb, seed=1, pad_frac=0.02, time_sorted=True)
        L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))
        g = torch.Generator().manual_seed(8)
        params = (torch.randn(B, 2 * d, H // 8, W // 8, generator=g) * 0.25).to(dev).requires_grad_(True)      # (x 8 in the upsampling: N(0, 2^2) pixels)
        mask = torch.randn(B, 576, H // 8, W // 8, generator=g).to(dev).requires_grad_(True)
        t_ref = torch.full((1,), 0.41, device=dev)
        times = torch.cat((t_ref, bin_mid_times(nb).to(dev)))
        sorted_b = {'events': ev.to(dev), 'num_pos_events': npos}
        batches = {'time_sorted': sorted_b, 'bucket_ordered': L.order_events(sorted_b)}
        sh = ops._pec_shape(L._cfg, sorted_b['events'], npos)
        table = None
        if args.curve != 'BEZIER':
            result['curve'], result['table_samples'] = args.curve, TABLE_SAMPLES
            table = utils.bspline_basis(torch.arange(TABLE_SAMPLES + 1, dtype=torch.float64) / TABLE_SAMPLES, d + 1).float().to(dev)
        kinds = {'BEZIER': ('BEZIER', None), 'BSPLINE': ('BSPLINE', 'TABLE'), 'TABLE': ('TABLE', 'BSPLINE')}[args.curve]

        def curve_kw(kind):
            return dict(curve_type=kind, basis_table=table if kind == 'TABLE' else None)
        out_w = {'desc': wl['desc'] + '; control points on the 1/8 grid + up_mask', 'sp': bench.SP, 'd': d,
                 'row_gradient_passes_ordered': int(C.lib().mpc_pec_rows_grad_passes(ctypes.byref(sh), d, 0)), 'layouts': {}}

        def clear():
            params.grad = None
            mask.grad = None

        for lname, b in batches.items():
            def r_fused():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, **curve_kw(kinds[0]))[0].backward()

            def r_fused_other():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, **curve_kw(kinds[1]))[0].backward()

            def r_unfused():
                L.calc_per_event_curves(params, t_ref, b, up_mask=mask, fused=False, **curve_kw(kinds[0]))[0].backward()

            def r_lut():
                if args.curve == 'BEZIER':
                    traj, _ = utils.trajectories_from_bezier(params, times, bench.PATCH, (H, W), up_mask=mask)
                else:
                    traj, _ = utils.trajectories_from_curves(params, times, bench.PATCH, (H, W), curve_type='BSPLINE', up_mask=mask)
                L.calc(traj, times, b)[0].backward()
            if args.curve == 'BEZIER':
                routes = {'fused': r_fused, 'unfused': r_unfused, 'lut': r_lut}
            else:
                routes = {'fused': r_fused, 'fused_other': r_fused_other, 'lut': r_lut}
            if args.routes:
                every = {'fused': r_fused, 'fused_other': r_fused_other, 'unfused': r_unfused, 'lut': r_lut}
                routes = {n: every[n] for n in args.routes.split(',') if n != 'fused_other' or kinds[1]}
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
                print(f'{wname} {lname} {n}: median {out[n]["median_ms"]} ms (min {out[n]["min_ms"]}, p90 {out[n]["p90_ms"]}); library kernels '
                      f'{out[n]["library_kernels_total_us"]} us: ' + ' '.join(f'{a}={v}' for a, v in list(ks.items())[:8]), flush=True)
            if args.curve != 'BEZIER' and lname == 'bucket_ordered' and 'fused' in routes:
                out['fused']['k_pec_accum_us_by_orders_per_pass'] = orders_per_pass_sweep(sh, d, r_fused, clear)
                print(f'{wname} {lname} k_pec_accum by orders per pass (0 = the library\'s choice): '
                      f'{out["fused"]["k_pec_accum_us_by_orders_per_pass"]}', flush=True)
            out_w['layouts'][lname] = out
        result['workloads'][wname] = out_w
        del batches, sorted_b, params, mask
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
