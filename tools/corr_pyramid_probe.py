#!/usr/bin/env python3
"""The fused RAFT-spline correlation pyramid (utils.corr_pyramid_fused -> ops.CorrPyramidFn, csrc/corr_pyramid.hip) against
utils.corr_pyramid (plain torch on the device: the reference's batched matmul, division and avg_pool2d chain) on the same GPU in ONE
process, the variants alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device synchronise.  The
shipped EVIMO2 shape: a 48 x 64 grid (384 x 512 / 8), feature dimension 256 (raft_base.yaml), 5 targets with levels [1, 1, 1, 1, 4], at
B = 1 and B = 6 (level 0 of the volume is 1.13 GB at B = 6).
  forward   the pyramid under no_grad
  fwd_bwd   forward + backward of fixed random level cotangents to both feature maps
The bar: on both legs and both batch sizes the fused median lies below the mirror's by more than the spread of the probe's own blocks
(the larger of the two variants' max - min).  Per-kernel times from the library's own events (mpc_profile_start / _stop), and the
fp32 FLOP/s the three GEMM launches achieve over the operations their shapes need (2 * B * D * hw * sum_l n_l h_l w_l each), beside
the 157.3 TF fp32 matrix peak.  Writes profiles/corr_pyramid.json (tagged with build.source_hash()):
    python tools/corr_pyramid_probe.py [out.json]
With --multi the reference's default model (raft-spline.yaml: use_boundary_images, a 384 x 512 input, so the same 48 x 64 grid and
D = 256): two references in list form, events [1, 2, 3, 4] plus frames [4] (ops.CorrPyramidMultiFn), against the list-form mirror --
the expand / cat, batched matmul, division and pool chain, which is what a caller had for this model before.  The same legs, bar
and per-kernel times, and per mode the peak rise of allocated device memory over one call.  Writes profiles/corr_pyramid_multi.json:
    python tools/corr_pyramid_probe.py --multi [out.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import utils, build, _lib as C  # noqa: E402

BLOCKS, CALLS, WARM = 7, 10, 2
H, W, D_FEAT, LEVELS = 48, 64, 256, [1, 1, 1, 1, 4]
LEVELS_MULTI = [[1, 2, 3, 4], [4]]                      # events, then frames
PEAK_TF = 157.3
GEMMS = {'k_corr_pyr_gemm<0>': 'forward', 'k_corr_pyr_gemm<1>': 'grad_pooled_fmap2', 'k_corr_pyr_gemm<2>': 'grad_fmap1'}
dev = torch.device('cuda:0')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / CALLS


def kernel_times(fn, reps):
    """{kernel name with its template argument: mean us per call of fn} from the library's events around every launch."""
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
        k = nm.strip().lstrip('(').rstrip(')').strip().replace(', T>', '>').replace('<T>', '')      # (the element type of a templated kernel)
        out[k] = out.get(k, 0.0) + 1e3 * t / reps
    return out


def peak_rise(fn):
    """Bytes by which the allocator's peak exceeds what is allocated before one call of fn (the results are dropped first)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - before)


def gemm_flops(B, levels):
    tix = utils.level_target_indices([v for ref in levels for v in ref] if isinstance(levels[0], list) else levels)
    return 2 * B * D_FEAT * H * W * sum(len(t) * (H >> l) * (W >> l) for l, t in enumerate(tix))


def main(out_path, levels=LEVELS):
    multi = isinstance(levels[0], list)
    if not torch.cuda.is_available():
        raise SystemExit('corr_pyramid_probe: no GPU; a timing on the CPU says nothing')
    res = {'source_hash': build.source_hash(), 'method': f'one process, variants alternating, median of {BLOCKS} blocks x {CALLS} calls after '
           f'{WARM} warm-up calls; host clock ending in torch.cuda.synchronize(); per-kernel: mpc_profile_start / mpc_profile_stop',
           'shape': dict(grid=[H, W], feature_dim=D_FEAT, num_levels_per_target=levels), 'fp32_matrix_peak_TF': PEAK_TF, 'batches': {}}
    for B in (1, 6):
        g = torch.Generator().manual_seed(256 + B)
        if multi:
            f1 = [torch.randn(B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True) for _ in levels]
            f2 = [torch.randn(len(ref), B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True) for ref in levels]
            leaves = f1 + f2
        else:
            f1 = torch.randn(B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
            f2 = torch.randn(len(levels), B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
            leaves = [f1, f2]
        with torch.no_grad():
            want, _ = utils.corr_pyramid(f1, f2, levels)
            got, _ = utils.corr_pyramid_fused(f1, f2, levels)
            cots = [torch.randn(lv.shape, device=dev) for lv in want]
            fwd_diff = [float((a - b).abs().max()) for a, b in zip(got, want)]
            level_bytes = 4 * sum(lv.numel() for lv in want)
            del want, got

        def fwd(f):
            def run():
                with torch.no_grad():
                    f(f1, f2, levels)
            return run

        def fwd_bwd(f):
            def run():
                return torch.autograd.grad(f(f1, f2, levels)[0], leaves, cots)
            return run

        modes = {'forward_mirror': fwd(utils.corr_pyramid), 'forward_fused': fwd(utils.corr_pyramid_fused),
                 'fwd_bwd_mirror': fwd_bwd(utils.corr_pyramid), 'fwd_bwd_fused': fwd_bwd(utils.corr_pyramid_fused)}
        ga, gb = modes['fwd_bwd_fused'](), modes['fwd_bwd_mirror']()
        grad_diff = [float((a - b).abs().max()) for a, b in zip(ga, gb)]
        grad_max = [float(b.abs().max()) for b in gb]
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
        kt = kernel_times(modes['fwd_bwd_fused'], 5)
        r['kernels_us'] = {k: round(v, 2) for k, v in sorted(kt.items())}
        if multi:
            r['peak_rise_bytes'] = {k: peak_rise(fn) for k, fn in modes.items()}
        flops = gemm_flops(B, levels)
        r['gemm_flops_each'] = flops
        r['gemm_achieved_TF'] = {GEMMS[k]: round(flops / (v * 1e-6) / 1e12, 1) for k, v in kt.items() if k in GEMMS}
        r['level_bytes'] = level_bytes
        if multi:
            r['max_abs_diff_to_mirror'] = dict(levels=fwd_diff, grad_fmap1=grad_diff[:len(levels)], grad_fmap2=grad_diff[len(levels):], max_abs_grad=grad_max)
        else:
            r['max_abs_diff_to_mirror'] = dict(levels=fwd_diff, grad_fmap1=grad_diff[0], grad_fmap2=grad_diff[1], max_abs_grad=grad_max)
        r['bar'] = {}
        for leg in ('forward', 'fwd_bwd'):
            a, m = r[leg + '_fused'], r[leg + '_mirror']
            margin = max(a['spread_ms'], m['spread_ms'])
            r['bar'][leg] = dict(gap_ms=round(m['median_ms'] - a['median_ms'], 4), margin_ms=margin,
                                 met=bool(m['median_ms'] - a['median_ms'] > margin))
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps({k: r[k]['median_ms'] for k in modes}), json.dumps(r['kernels_us']), json.dumps(r['gemm_achieved_TF']),
              json.dumps(r['bar']), json.dumps(r['max_abs_diff_to_mirror']), flush=True)
        del cots, modes, f1, f2, leaves
        torch.cuda.empty_cache()
    res['bar_met_on_every_leg'] = all(leg['met'] for b in res['batches'].values() for leg in b['bar'].values())
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out_path)


if __name__ == '__main__':
    argv = [a for a in sys.argv[1:] if a != '--multi']
    if '--multi' in sys.argv[1:]:
        main(argv[0] if argv else os.path.join(ROOT, 'profiles', 'corr_pyramid_multi.json'), LEVELS_MULTI)
    else:
        main(argv[0] if argv else os.path.join(ROOT, 'profiles', 'corr_pyramid.json'))
