#!/usr/bin/env python3
"""The RAFT-spline correlation lookup node (utils.CorrLookup.lookup_bezier -> ops.CorrLookupFn, csrc/corr_lookup.hip) against its
plain-torch mirror (utils/corr.py: the reference's coordinate tensor / grid_sample / cat / permute chain) on the same GPU in ONE
process, the variants alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device synchronise.  The
shipped EVIMO2 shape: a 48 x 64 grid (384 x 512 / 8), d = 10, 5 targets with levels [1, 1, 1, 1, 4] (8 entries), radius 4, at B = 1 and
B = 6 (level 0 of the volume is 1.13 GB at B = 6).
  forward          the lookup under no_grad
  fwd_bwd_params   forward + backward of a fixed cotangent to params
  fwd_bwd_all      forward + backward to params and every level
  twelve_forwards  twelve forwards in a row: what one forward of the network does (raft.py:165-189)
each for the fused node, the mirror, and -- forward cases -- the fused node with the lane-per-query forward
(MPC_CORR_F_LANE_PER_QUERY: the window mapping that lost).  Per-kernel times from ops.KernelTimer and the rate they amount to over the bytes the algorithm needs: the
output plus E * (2r + 2)^2 floats per query.  Writes profiles/corr_lookup.json (tagged with build.source_hash()):
    python tools/corr_lookup_probe.py [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import ops, utils, build, _lib as C  # noqa: E402
from motionpriorcmax_amd.utils import corr as uc  # noqa: E402

BLOCKS, CALLS, WARM = 7, 10, 2
H, W, D_FEAT, D, LEVELS, R = 48, 64, 16, 10, [1, 1, 1, 1, 4], 4
TIMES = [0.2, 0.4, 0.6, 0.8, 1.0]
dev = torch.device('cuda:0')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / CALLS


def algorithmic_bytes(B):
    E, K, q = sum(LEVELS), 2 * R + 1, B * H * W
    out, windows = 4 * q * E * K * K, 4 * q * E * (K + 1) ** 2
    return dict(forward=out + windows, output=out, windows=windows)


def main(out_path):
    res = {'source_hash': build.source_hash(), 'method': f'one process, variants alternating, median of {BLOCKS} blocks x {CALLS} calls after '
           f'{WARM} warm-up calls; host clock ending in torch.cuda.synchronize(); per-kernel: ops.KernelTimer',
           'shape': dict(grid=[H, W], d=D, times=TIMES, num_levels_per_target=LEVELS, radius=R, feature_dim=D_FEAT), 'batches': {}}
    for B in (1, 6):
        g = torch.Generator().manual_seed(16 + B)
        f1 = torch.randn(B, D_FEAT, H, W, generator=g).to(dev)
        f2 = torch.randn(len(LEVELS), B, D_FEAT, H, W, generator=g).to(dev)
        levels, _ = utils.corr_pyramid(f1, f2, LEVELS)
        del f1, f2
        frozen = utils.CorrLookup([lv.detach() for lv in levels], LEVELS, radius=R)
        lane = utils.CorrLookup(frozen.levels, LEVELS, radius=R)
        lane.flags = C.CORR_F_LANE_PER_QUERY
        leaves = utils.CorrLookup([lv.detach().requires_grad_(True) for lv in levels], LEVELS, radius=R)
        p = (torch.randn(B, 2 * D, H, W, generator=g) * 3.0).to(dev).requires_grad_(True)
        K = 2 * R + 1
        go = torch.randn(B, sum(LEVELS) * K * K, H, W, generator=g).to(dev)
        bm = frozen._basis(TIMES, D, dev, torch.float32)
        grid = uc.coords_grid(B, H, W, dev)

        def fused(lk):
            return lambda: lk.lookup_bezier(p, TIMES)

        def mirror(lk):
            def run():
                flows = torch.einsum('bcdhw,td->tbchw', p.reshape(B, 2, D, H, W), bm)
                return uc._lookup_mirror(lk.levels, lk.target_indices, R, grid[None] + flows)
            return run

        def fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def twelve(f):
            def run():
                with torch.no_grad():
                    for _ in range(12):
                        f()
            return run

        def fwd_bwd(f, lk, with_levels):
            ins = [p] + (list(lk.levels) if with_levels else [])

            def run():
                torch.autograd.grad(f(), ins, go)
            return run

        modes = {
            'forward_mirror': fwd(mirror(frozen)), 'forward_fused': fwd(fused(frozen)), 'forward_fused_lane_per_query': fwd(fused(lane)),
            'fwd_bwd_params_mirror': fwd_bwd(mirror(frozen), frozen, False), 'fwd_bwd_params_fused': fwd_bwd(fused(frozen), frozen, False),
            'fwd_bwd_all_mirror': fwd_bwd(mirror(leaves), leaves, True), 'fwd_bwd_all_fused': fwd_bwd(fused(leaves), leaves, True),
            'twelve_forwards_mirror': twelve(mirror(frozen)), 'twelve_forwards_fused': twelve(fused(frozen)),
            'twelve_forwards_fused_lane_per_query': twelve(fused(lane)),
        }
        with torch.no_grad():                                    # the two forwards agree bit for bit, the mirror within 1e-4
            a, b, m = fused(frozen)(), fused(lane)(), mirror(frozen)()
            same_bits, mirror_diff = bool(torch.equal(a, b)), float((a - m).abs().max())
            del a, b, m
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
                modes['fwd_bwd_all_fused']()
                modes['fwd_bwd_params_fused']()
                modes['forward_fused_lane_per_query']()
        ks = kt.summary()
        with ops.KernelTimer() as kt2:
            for _ in range(5):
                modes['fwd_bwd_params_fused']()
        r['kernels'] = {'k_corr_lookup_fwd': round(ks['k_corr_lookup_fwd']['avg_us'], 2),
                        'k_corr_lookup_fwd_lane': round(ks['k_corr_lookup_fwd_lane']['avg_us'], 2),
                        'k_corr_lookup_bwd_params_only': round(kt2.summary()['k_corr_lookup_bwd']['avg_us'], 2),
                        'k_corr_lookup_bwd_params_and_levels': round((ks['k_corr_lookup_bwd']['total_us'] - kt2.summary()['k_corr_lookup_bwd']['total_us']) / 5, 2)}
        zero_ms = statistics.median(timed(lambda: [torch.zeros_like(lv) for lv in levels]) for _ in range(BLOCKS))
        r['zero_fill_of_the_level_gradients_ms'] = round(zero_ms, 4)          # the yardstick of the backward's slice fill: the same bytes, zeros only
        by = algorithmic_bytes(B)
        by['grad_levels'] = 4 * sum(lv.numel() for lv in levels)
        r['bytes'] = by
        r['achieved_GBps'] = dict(forward=round(by['forward'] / r['kernels']['k_corr_lookup_fwd'] / 1e3, 1),
                                  forward_lane_per_query=round(by['forward'] / r['kernels']['k_corr_lookup_fwd_lane'] / 1e3, 1),
                                  backward_params_and_levels=round((by['forward'] + by['grad_levels']) / r['kernels']['k_corr_lookup_bwd_params_and_levels'] / 1e3, 1))
        r['forwards_agree_bitwise'], r['max_abs_diff_to_mirror'] = same_bits, mirror_diff
        r['fused_faster_than_mirror'] = {c: bool(r[c + '_fused']['median_ms'] < r[c + '_mirror']['median_ms'])
                                         for c in ('forward', 'fwd_bwd_params', 'fwd_bwd_all', 'twelve_forwards')}
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps({k: r[k]['median_ms'] for k in modes}), json.dumps(r['kernels']), json.dumps(r['achieved_GBps']),
              json.dumps(r['fused_faster_than_mirror']), same_bits, mirror_diff, flush=True)
        del levels, frozen, lane, leaves, modes
        torch.cuda.empty_cache()
    res['keeps_the_node'] = all(all(b['fused_faster_than_mirror'].values()) for b in res['batches'].values())
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out_path)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'corr_lookup.json'))
