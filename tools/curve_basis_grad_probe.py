#!/usr/bin/env python3
"""The RAFT-spline refinement loop with a LEARNED curve whose basis network trains: `basis_grad='mirror'` (the plain-torch mirrors, the
behaviour without the keyword) against `basis_grad='fused'` (the fused nodes, the matrix' gradient by csrc/curve_basis.hip), and the
frozen network on this tree's library and -- with --parent-lib -- on the parent commit's library loaded beside it.  One process, the
legs alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device synchronise (the method of
tools/corr_loop_probe.py).  The shipped EVIMO2 shape: a 48 x 64 grid, feature dimension 256, 5 targets with levels [1, 1, 1, 1, 4],
radius 4, d = 10; a call is utils.CorrLookup.from_fmaps, 12 chained lookup_curves, the convex-upsampling head
(trajectories_from_curves with up_mask, tile 4, 42 times) and the backward to the feature maps, the control points, the mask and --
in the two training legs -- the parameters of the reference's basis network (1 -> 64 -> 64 -> d), at B = 1 and B = 6.
The criterion at each batch size: `fused` lies below `mirror` by more than the margin, the larger max - min over the blocks of the two
legs.  The regression check: the frozen leg on this library against the parent's within the margin of those two legs.  Also reported:
per-kernel times of the library's kernels through ops.KernelTimer (torch's own kernels show in the host clock alone), what the
matrix' gradient costs over the frozen route (the extra launches' microseconds, the bytes of grad_coords written), the peak of
torch.cuda.max_memory_allocated over one call of each leg.  Writes profiles/curve_basis_grad.json (tagged with build.source_hash()):
    python tools/curve_basis_grad_probe.py [--parent-lib /path/to/parent/libmpcmax.so] [out.json]"""
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

from motionpriorcmax_amd import utils, ops, build, _lib as C  # noqa: E402

BLOCKS, CALLS, WARM = 7, 10, 2
H, W, D_FEAT, LEVELS, RADIUS, D_CTRL, ITERS = 48, 64, 256, [1, 1, 1, 1, 4], 4, 10, 12
HEAD_TILE, HEAD_TIMES = 4, 42
EXTRA_KERNELS = ('k_curve_basis_part', 'k_curve_basis_sum', 'k_pec_head_rows')
dev = torch.device('cuda:0')


def load_parent(path):
    """The parent commit's library with the binding's signatures on every symbol it has (it lacks the reduction's two)."""
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in C.SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return L


class using:
    """The binding's calls go into `handle` inside (None: this tree's library)."""

    def __init__(self, handle):
        self.handle = handle

    def __enter__(self):
        self.own = C.lib()
        if self.handle is not None:
            C._lib = self.handle

    def __exit__(self, *exc):
        C._lib = self.own
        return False


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / CALLS


def basis_network():
    """Reference src/modules/raft_spline.py:29-34."""
    torch.manual_seed(7)
    return torch.nn.Sequential(torch.nn.Linear(1, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, D_CTRL)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'curve_basis_grad.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('curve_basis_grad_probe: no GPU; a timing on the CPU says nothing')
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    res = {'source_hash': build.source_hash(), 'parent_library': bool(a.parent_lib), 'device': torch.cuda.get_device_name(0),
           'method': f'one process, legs alternating, median of {BLOCKS} blocks x {CALLS} calls after {WARM} warm-up calls; host clock ending in '
                     'torch.cuda.synchronize(); per-kernel: ops.KernelTimer over 3 calls; margin: the larger max - min over the blocks of the two legs compared',
           'shape': dict(grid=[H, W], feature_dim=D_FEAT, num_levels_per_target=LEVELS, radius=RADIUS, d=D_CTRL, lookups=ITERS,
                         head=dict(tile=HEAD_TILE, times=HEAD_TIMES, image=[8 * H, 8 * W]), basis_network='1 -> 64 -> 64 -> d'), 'batches': {}}
    times = torch.tensor([(i + 1) / len(LEVELS) for i in range(len(LEVELS))], device=dev)
    head_times = torch.linspace(0.0, 1.0, HEAD_TIMES, device=dev)
    K = 2 * RADIUS + 1
    n_head = (8 * H // HEAD_TILE) * (8 * W // HEAD_TILE)
    for B in (1, 6):
        g = torch.Generator().manual_seed(2100 + B)
        f1 = torch.randn(B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
        f2 = torch.randn(len(LEVELS), B, D_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
        p0 = (torch.randn(B, 2 * D_CTRL, H, W, generator=g) * 3.0).to(dev).requires_grad_(True)
        mask = torch.randn(B, 576, H, W, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, sum(LEVELS) * K * K, H, W, generator=g).to(dev)
        gt = torch.randn(B, HEAD_TIMES, n_head, 2, generator=g).to(dev)
        nets = {'train': basis_network(), 'frozen': basis_network().requires_grad_(False)}

        def loop(route, net):
            def run():
                lk = utils.CorrLookup.from_fmaps(f1, f2, LEVELS, radius=RADIUS)
                p, outs = p0, []
                for _ in range(ITERS):
                    out = lk.lookup_curves(p, times, 'LEARNED', net, basis_grad=route)
                    outs.append(out)
                    p = p + 0.01 * out[:, :2 * D_CTRL]
                traj, _ = utils.trajectories_from_curves(p, head_times, HEAD_TILE, (8 * H, 8 * W), 'LEARNED', net, scale=8.0, up_mask=mask, basis_grad=route)
                wrt = [f1, f2, p0, mask] + [q for q in net.parameters() if q.requires_grad]
                return torch.autograd.grad(outs + [traj], wrt, [go] * ITERS + [gt])
            return run

        legs = {'mirror': (None, loop('mirror', nets['train'])), 'fused': (None, loop('fused', nets['train'])),
                'frozen': (None, loop('mirror', nets['frozen']))}
        if parent is not None:
            legs['frozen_parent'] = (parent, loop('mirror', nets['frozen']))
        gm, gf, gz = legs['mirror'][1](), legs['fused'][1](), legs['frozen'][1]()
        r = {'fused_equals_frozen_bitwise': dict(zip(('grad_fmap1', 'grad_fmap2', 'grad_params', 'grad_mask'), (bool(torch.equal(x, y)) for x, y in zip(gf, gz)))),
             'fused_against_mirror_network_gradients_max_rel': [round(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)), 9) for x, y in zip(gf[4:], gm[4:])]}
        del gm, gf, gz
        for lib, fn in legs.values():
            with using(lib):
                for _ in range(WARM):
                    fn()
        samples = {k: [] for k in legs}
        for _ in range(BLOCKS):
            for k, (lib, fn) in legs.items():
                with using(lib):
                    samples[k].append(timed(fn))
        for k, v in samples.items():
            r[k] = {'median_ms': round(statistics.median(v), 4), 'spread_ms': round(max(v) - min(v), 4), 'blocks_ms': [round(x, 4) for x in v]}
        for k, (lib, fn) in legs.items():
            if lib is not None:
                continue
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
        fk, zk = r['fused']['kernels'], r['frozen']['kernels']
        r['basis_gradient_cost_over_frozen'] = dict(
            extra_launches_per_call=sum(fk[n]['launches_per_call'] for n in EXTRA_KERNELS if n in fk),
            extra_kernels_us_per_call=round(sum(fk[n]['total_us_per_call'] for n in EXTRA_KERNELS if n in fk), 1),
            lookup_bwd_us_per_call=dict(fused=fk['k_corr_lookup_bwd']['total_us_per_call'], frozen=zk['k_corr_lookup_bwd']['total_us_per_call']),
            grad_coords_bytes_written_per_call=ITERS * len(LEVELS) * B * 2 * H * W * 4,
            library_kernels_us_per_call=dict(fused=r['fused']['library_kernels_us_per_call'], frozen=r['frozen']['library_kernels_us_per_call']),
            host_clock_ms=round(r['fused']['median_ms'] - r['frozen']['median_ms'], 4))
        margin = max(r['fused']['spread_ms'], r['mirror']['spread_ms'])
        r['criterion'] = dict(gap_ms=round(r['mirror']['median_ms'] - r['fused']['median_ms'], 4), margin_ms=margin,
                              met=bool(r['mirror']['median_ms'] - r['fused']['median_ms'] > margin))
        if parent is not None:
            margin = max(r['frozen']['spread_ms'], r['frozen_parent']['spread_ms'])
            diff = r['frozen']['median_ms'] - r['frozen_parent']['median_ms']
            r['regression_check'] = dict(frozen_minus_parent_ms=round(diff, 4), margin_ms=margin, within_margin=bool(abs(diff) <= margin))
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps({k: r[k]['median_ms'] for k in legs}), json.dumps(r['criterion']), json.dumps(r.get('regression_check')),
              json.dumps(r['basis_gradient_cost_over_frozen']), flush=True)
        for k in legs:
            if 'kernels' in r[k]:
                print(' ', k, r[k]['peak_rise_bytes'], json.dumps(r[k]['kernels']), flush=True)
        print(' ', json.dumps(r['fused_equals_frozen_bitwise']), r['fused_against_mirror_network_gradients_max_rel'], flush=True)
        del legs, f1, f2, p0, mask, go, gt, nets
        torch.cuda.empty_cache()
    res['criterion_met_at_every_batch'] = all(b['criterion']['met'] for b in res['batches'].values())
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
