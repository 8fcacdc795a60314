#!/usr/bin/env python3
"""The RAFT-spline refinement loop's correlation path with `shared_grad` off against on (utils.CorrLookup.from_fmaps: ops.CorrPyramidFn,
then 12 chained lookup_bezier calls, then the backward to both feature maps and the control points), on the same GPU in ONE process,
the variants alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device synchronise (the method of
tools/corr_pyramid_probe.py).  The shipped EVIMO2 shape: a 48 x 64 grid, feature dimension 256, 5 targets with levels [1, 1, 1, 1, 4],
radius 4, d = 10, at B = 1 and B = 6.
  off   every lookup backward returns a whole level set (window cells + zeros), autograd adds the twelve
  on    the twelve add their window cells into one set (ops.CorrGradGateFn / CorrLookupSharedFn, MPC_CORR_F_GRAD_ACCUM)
The bar for recommending the mode: at both batch sizes `on` lies below `off` by more than the spread of the probe's own blocks (the
larger of the two variants' max - min).  Per-kernel times of the library's kernels through ops.KernelTimer (torch's own kernels, the
adds of `off` among them, are not in it: they show in the host clock alone), the backward kernel split by its template arguments
(fill / accumulate) through the library's events, and the peak of torch.cuda.max_memory_allocated over one call of each variant.
Writes profiles/corr_loop.json (tagged with build.source_hash()):
    python tools/corr_loop_probe.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import utils, ops, build, _lib as C  # noqa: E402

BLOCKS, CALLS, WARM = 7, 10, 2
H, W, D_FEAT, LEVELS, RADIUS, D_CTRL, ITERS = 48, 64, 256, [1, 1, 1, 1, 4], 4, 10, 12
dev = torch.device('cuda:0')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / CALLS


def split_kernel_times(fn, reps):
    """{kernel name WITH its template arguments: (launches per call, mean us per launch)} from the library's events."""
    L = C.lib()
    torch.cuda.synchronize()
    L.mpc_profile_start()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    cap = 1 << 14
    names = ctypes.create_string_buffer(cap * 48)
    ms = (ctypes.c_float * cap)()
    n = int(L.mpc_profile_stop(names, len(names), ms, cap))
    out = {}
    for nm, t in zip(names.value.decode().split('\n')[:n], ms[:n]):
        k = nm.strip().lstrip('(').rstrip(')').strip()
        r = out.setdefault(k, [0, 0.0])
        r[0] += 1
        r[1] += 1e3 * t
    return {k: dict(launches_per_call=v[0] / reps, avg_us=round(v[1] / v[0], 2)) for k, v in sorted(out.items())}


def main(out_path):
    if not torch.cuda.is_available():
        raise SystemExit('corr_loop_probe: no GPU; a timing on the CPU says nothing')
    res = {'source_hash': build.source_hash(), 'method': f'one process, variants alternating, median of {BLOCKS} blocks x {CALLS} calls after '
           f'{WARM} warm-up calls; host clock ending in torch.cuda.synchronize(); per-kernel: ops.KernelTimer over 3 calls',
           'shape': dict(grid=[H, W], feature_dim=D_FEAT, num_levels_per_target=LEVELS, radius=RADIUS, d=D_CTRL, lookups=ITERS), 'batches': {}}
    times = [(i + 1) / len(LEVELS) for i in range(len(LEVELS))]
    K = 2 * RADIUS + 1
    for B in (1, 6):
        g = torch.Generator().manual_seed(1200 + B)
        f1 = torch.randn(B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
        f2 = torch.randn(len(LEVELS), B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
        p0 = (torch.randn(B, 2 * D_CTRL, H, W, generator=g) * 3.0).to(dev).requires_grad_(True)
        go = torch.randn(B, sum(LEVELS) * K * K, H, W, generator=g).to(dev)

        def loop(shared):
            def run():
                lk = utils.CorrLookup.from_fmaps(f1, f2, LEVELS, radius=RADIUS, shared_grad=shared)
                p, outs = p0, []
                for _ in range(ITERS):
                    out = lk.lookup_bezier(p, times)
                    outs.append(out)
                    p = p + 0.01 * out[:, :2 * D_CTRL]
                return torch.autograd.grad(outs, [f1, f2, p0], [go] * ITERS)
            return run

        modes = {'off': loop(False), 'on': loop(True)}
        ga, gb = modes['off'](), modes['on']()
        equal = [bool(torch.equal(a, b)) for a, b in zip(ga, gb)]
        with torch.no_grad():
            level_bytes = 4 * sum(lv.numel() for lv in utils.corr_pyramid_fused(f1, f2, LEVELS)[0])
        del ga, gb
        for fn in modes.values():
            for _ in range(WARM):
                fn()
        samples = {k: [] for k in modes}
        for _ in range(BLOCKS):
            for k, fn in modes.items():
                samples[k].append(timed(fn))
        r = {k: {'median_ms': round(statistics.median(v), 4), 'spread_ms': round(max(v) - min(v), 4), 'blocks_ms': [round(x, 4) for x in v]}
             for k, v in samples.items()}
        for k, fn in modes.items():
            with ops.KernelTimer() as kt:
                for _ in range(3):
                    fn()
            r[k]['kernels'] = {n: dict(launches_per_call=v['launches'] / 3, avg_us=round(v['avg_us'], 2), total_us_per_call=round(v['total_us'] / 3, 1))
                               for n, v in sorted(kt.summary().items())}
            r[k]['library_kernels_us_per_call'] = round(sum(v['total_us'] for v in kt.summary().values()) / 3, 1)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            r[k]['peak_allocated_bytes'] = int(torch.cuda.max_memory_allocated())
            r[k]['peak_rise_bytes'] = int(torch.cuda.max_memory_allocated() - base)
        r['on']['backward_kernel_by_role'] = {n: v for n, v in split_kernel_times(modes['on'], 3).items() if 'k_corr_lookup_bwd' in n}
        r['level_set_bytes'] = level_bytes
        r['gradients_bitwise_equal'] = dict(zip(('grad_fmap1', 'grad_fmap2', 'grad_params'), equal))
        margin = max(r['on']['spread_ms'], r['off']['spread_ms'])
        r['bar'] = dict(gap_ms=round(r['off']['median_ms'] - r['on']['median_ms'], 4), margin_ms=margin,
                        met=bool(r['off']['median_ms'] - r['on']['median_ms'] > margin))
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps({k: r[k]['median_ms'] for k in modes}), json.dumps(r['bar']),
              json.dumps({k: r[k]['peak_rise_bytes'] for k in modes}), json.dumps(r['gradients_bitwise_equal']), flush=True)
        for k in modes:
            print(' ', k, json.dumps(r[k]['kernels']), flush=True)
        print('  on, by role', json.dumps(r['on']['backward_kernel_by_role']), flush=True)
        del modes, f1, f2, p0, go
        torch.cuda.empty_cache()
    res['bar_met_at_every_batch'] = all(b['bar']['met'] for b in res['batches'].values())
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out_path)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'corr_loop.json'))
