#!/usr/bin/env python3
"""The correlation pyramid from bf16 feature maps (include/mpcmax.h: mpc_corr_pyramid_*_dt; level 0 of the forward on
v_mfma_f32_32x32x16_bf16) against the route a caller had before it -- the reference's own `.float()` (raft.py:126) in front of the
fp32 node.  The shipped EVIMO2 shape of tools/corr_pyramid_probe.py (48 x 64 grid, D = 256, levels [1, 1, 1, 1, 4]) at B = 1 and B = 6,
ONE process, the legs alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device synchronise.
  legs     upcast          bf16 maps -> .float() -> the fp32 node (this tree's library); the backward ends in autograd's cast of the fp32
                           gradients back to bf16
           upcast_parent   the same with the fp32 node's calls made into the PARENT commit's library (--parent-lib: a second
                           libmpcmax.so in the process, its fp32 entry points bound here by hand)
           native          the bf16 maps handed to the node as they are
           fill            forward only: a plain fill of the same level bytes (preallocated): the write floor of a forward
  each as `forward` (no_grad) and `fwd_bwd` (fixed random level cotangents, gradients to both bf16 maps)
  spread   per leg max - min over its blocks; a comparison's margin is the larger spread of its two legs
  checks   forward: native < baseline - margin;  fwd_bwd: native <= baseline + margin;  fp32 route: |upcast - upcast_parent| <= margin
           (baseline: upcast_parent where a parent library is given, else upcast)
Per-kernel times of the native and the upcast leg from the library's own events, the peak rise of allocated device memory over one
call per leg, the forward against the fill, the achieved TF/s of the level-0 launch (2 B D hw T hw operations) and the share of the
levels >= 1 (their pools and their GEMM launch) in the native forward's kernel time.  Writes profiles/corr_pyramid_half.json:
    python tools/corr_pyramid_half_probe.py --parent-lib /path/to/parent/libmpcmax.so [out.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

import corr_pyramid_probe as base  # noqa: E402
from motionpriorcmax_amd import ops, utils, build, _lib as C  # noqa: E402

H, W, D_FEAT, LEVELS = base.H, base.W, base.D_FEAT, base.LEVELS
BLOCKS, WARM = base.BLOCKS, base.WARM
PEAK_16BIT_TF = 2516.6                       # dense bf16 / fp16 matrix peak of the MI355X
dev = torch.device('cuda:0')
PARENT = None                                # ctypes handle of the parent commit's library


def load_parent(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ('mpc_corr_pyramid_fwd', 'mpc_corr_pyramid_bwd', 'mpc_corr_pyramid_workspace_bytes', 'mpc_version'):
        getattr(L, name).restype, getattr(L, name).argtypes = C.SIGNATURES[name]
    assert L.mpc_version() == 107
    return L


class ParentCorrPyramidFn(torch.autograd.Function):
    """ops.CorrPyramidFn for fp32 maps with a cotangent at every level, its calls made into the parent commit's library."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, nl):
        T, B, D, h, w = fmap2.shape
        desc, tix = ops.corr_pyramid_desc(B, h, w, nl)
        levels = [torch.empty((len(ts), B * h * w, 1, h >> l, w >> l), dtype=torch.float32, device=fmap1.device) for l, ts in enumerate(tix)]
        f1, f2 = fmap1.detach(), fmap2.detach()
        for l, lv in enumerate(levels):
            desc.level[l] = lv.data_ptr()
        ws = torch.empty((PARENT.mpc_corr_pyramid_workspace_bytes(ctypes.byref(desc), D, 0) + 3) // 4, dtype=torch.float32, device=f1.device)
        rc = PARENT.mpc_corr_pyramid_fwd(ctypes.byref(desc), D, ops._ptr(f1), ops._ptr(f2), ops._ptr(ws), ops._stream(f1.device))
        assert rc == 0, rc
        ctx.nl = nl
        ctx.save_for_backward(f1, f2)
        return tuple(levels)

    @staticmethod
    def backward(ctx, *gl):
        f1, f2 = ctx.saved_tensors
        T, B, D, h, w = f2.shape
        g1, g2 = torch.empty_like(f1), torch.empty_like(f2)
        desc, _ = ops.corr_pyramid_desc(B, h, w, ctx.nl)
        gl = [g.contiguous() for g in gl]
        for l, g in enumerate(gl):
            desc.grad_level[l] = g.data_ptr()
        ws = torch.empty((PARENT.mpc_corr_pyramid_workspace_bytes(ctypes.byref(desc), D, 1) + 3) // 4, dtype=torch.float32, device=f1.device)
        rc = PARENT.mpc_corr_pyramid_bwd(ctypes.byref(desc), D, ops._ptr(f1), ops._ptr(f2), ops._ptr(g1), ops._ptr(g2), ops._ptr(ws),
                                         ops._stream(f1.device))
        assert rc == 0, rc
        return g1, g2, None


def run_batch(B):
    g = torch.Generator().manual_seed(256 + B)
    f1 = torch.randn(B, D_FEAT, H, W, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    f2 = torch.randn(len(LEVELS), B, D_FEAT, H, W, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    routes = {'upcast': lambda: utils.corr_pyramid_fused(f1.float(), f2.float(), LEVELS)[0],
              'native': lambda: utils.corr_pyramid_fused(f1, f2, LEVELS)[0]}
    if PARENT is not None:
        routes['upcast_parent'] = lambda: list(ParentCorrPyramidFn.apply(f1.float(), f2.float(), LEVELS))
    with torch.no_grad():
        want = routes['upcast']()
        got = routes['native']()
        assert all(lv.dtype == torch.float32 for lv in got)
        cots = [torch.randn(lv.shape, device=dev) for lv in want]
        fills = [torch.empty_like(lv) for lv in want]
        level_bytes = 4 * sum(lv.numel() for lv in want)
        diff = dict(level0_max_abs=float((got[0] - want[0]).abs().max()), level0_max=float(want[0].abs().max()),
                    levels_above_bitwise=all(torch.equal(a, b) for a, b in zip(got[1:], want[1:])))
        if PARENT is not None:
            diff['fp32_route_equals_parent_bitwise'] = all(torch.equal(a, b) for a, b in zip(routes['upcast_parent'](), want))
        del want, got

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            return torch.autograd.grad(f(), [f1, f2], cots)
        return run

    def fill():
        for t in fills:
            t.fill_(1.0)

    modes = {'forward_fill': fill}
    for k, f in routes.items():
        modes['forward_' + k], modes['fwd_bwd_' + k] = fwd(f), fwd_bwd(f)
    ga, gb = modes['fwd_bwd_native'](), modes['fwd_bwd_upcast']()
    diff['gradients_bitwise'] = all(a.dtype == torch.bfloat16 and torch.equal(a, b) for a, b in zip(ga, gb))
    del ga, gb
    for fn in modes.values():
        for _ in range(WARM):
            fn()
    samples = {k: [] for k in modes}
    for _ in range(BLOCKS):
        for k, fn in modes.items():
            samples[k].append(base.timed(fn))
    r = {k: {'median_ms': round(statistics.median(v), 4), 'spread_ms': round(max(v) - min(v), 4), 'blocks_ms': [round(x, 4) for x in v]}
         for k, v in samples.items()}
    r['kernels_us'] = {leg: {k: round(v, 2) for k, v in sorted(base.kernel_times(modes[leg], 5).items())}
                       for leg in ('forward_native', 'fwd_bwd_native', 'forward_upcast', 'fwd_bwd_upcast')}
    r['peak_rise_bytes'] = {k: base.peak_rise(fn) for k, fn in modes.items() if k != 'forward_fill'}
    r['level_bytes'] = level_bytes
    r['differences'] = diff
    kf = r['kernels_us']['forward_native']
    flops0 = 2 * B * D_FEAT * H * W * len(LEVELS) * H * W
    above = sum(v for k, v in kf.items() if k.startswith('k_corr_pyr_pool') or k.startswith('k_corr_pyr_gemm<0>'))
    r['report'] = dict(forward_native_over_fill=round(r['forward_native']['median_ms'] / r['forward_fill']['median_ms'], 3),
                       fill_TB_per_s=round(level_bytes / (r['forward_fill']['median_ms'] * 1e-3) / 1e12, 3),
                       level0_launch_us=kf.get('k_corr_pyr_gemm16'), level0_flops=flops0,
                       level0_achieved_TF=round(flops0 / (kf['k_corr_pyr_gemm16'] * 1e-6) / 1e12, 1),
                       level0_write_TB_per_s=round(4 * B * H * W * len(LEVELS) * H * W / (kf['k_corr_pyr_gemm16'] * 1e-6) / 1e12, 3),
                       levels_above_0_us=round(above, 2), levels_above_0_share=round(above / sum(kf.values()), 4))
    basel = 'upcast_parent' if PARENT is not None else 'upcast'
    chk = {}
    for leg, faster in (('forward', True), ('fwd_bwd', False)):
        a, m = r[f'{leg}_native'], r[f'{leg}_{basel}']
        margin = max(a['spread_ms'], m['spread_ms'])
        gap = round(m['median_ms'] - a['median_ms'], 4)
        chk[leg] = dict(baseline=basel, gap_ms=gap, margin_ms=margin, met=bool(gap > margin if faster else gap >= -margin))
        if PARENT is not None:
            a, m = r[f'{leg}_upcast'], r[f'{leg}_upcast_parent']
            margin = max(a['spread_ms'], m['spread_ms'])
            gap = round(a['median_ms'] - m['median_ms'], 4)
            chk[leg + '_fp32_route_vs_parent'] = dict(gap_ms=gap, margin_ms=margin, met=bool(abs(gap) <= margin))
    r['checks'] = chk
    return r


def main():
    global PARENT
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'corr_pyramid_half.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('corr_pyramid_half_probe: no GPU; a timing on the CPU says nothing')
    if a.parent_lib:
        PARENT = load_parent(a.parent_lib)
    res = {'source_hash': build.source_hash(), 'parent_library': bool(a.parent_lib),
           'method': f'one process, legs alternating, median of {BLOCKS} blocks x {base.CALLS} calls after {WARM} warm-up calls; host clock ending in '
                     'torch.cuda.synchronize(); per-kernel: mpc_profile_start / mpc_profile_stop; margin of a comparison: the larger max - min of its two legs',
           'shape': dict(grid=[H, W], feature_dim=D_FEAT, num_levels_per_target=LEVELS, dtype='bfloat16'),
           'matrix_peak_TF': dict(fp32=base.PEAK_TF, bf16=PEAK_16BIT_TF), 'batches': {}}
    for B in (1, 6):
        r = res['batches'][f'B{B}'] = run_batch(B)
        print(f'B={B}', json.dumps({k: v['median_ms'] for k, v in r.items() if isinstance(v, dict) and 'median_ms' in v}),
              json.dumps(r['report']), json.dumps(r['checks']), json.dumps(r['differences']), flush=True)
        torch.cuda.empty_cache()
    res['checks_met'] = all(c['met'] for b in res['batches'].values() for c in b['checks'].values())
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
