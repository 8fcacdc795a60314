#!/usr/bin/env python3
"""bf16 network tensors in the head nodes (include/mpcmax.h: the `_dt` entry points) against the route a user had to write before them:
x.float() -> the fp32 node -> autograd's cast of the dense fp32 gradient back to bf16.  ONE process, the legs alternating inside every
block; a time is the device-event time of a block of steps divided by the steps, a leg's figure the median over the blocks, and every
leg's blocks are in the file, so the run-to-run spread is too.
  shapes   C3 grid [14, 1, 6, 480, 640], polynomial k = 3, 16 times; C4 head B = 6, d = 10, 48 x 64 cells, tile 4, 42 times
  legs     native          the bf16 tensor handed to the node as it is (this tree's library)
           upcast          x.float() -> the fp32 node -> the cast back, on this tree's library
           upcast_parent   the same with the fp32 node's two calls made into the PARENT commit's library (--parent-lib: a second
                           libmpcmax.so in the process, its fp32 entry points bound here by hand -- the binding of this tree needs the
                           `_dt` symbols, so MPC_AB_LIB cannot load that library as the product one)
           fp32, fp32_parent   an fp32 tensor through the fp32 node, on either library (the fp32 route must not have moved)
           step_*          C3 only: the whole step from the grid -- times, node, FocusLoss.calc, backward to the grid
  spread   max - min over the blocks of the parent's leg (upcast_parent, fp32_parent), per shape
  accept   native <= upcast_parent + spread;  |fp32 - fp32_parent| <= spread
Per-kernel times of the native and the upcast leg: ops.KernelTimer (the library's own profile; torch's cast kernels are not in it).
    python tools/half_heads_probe.py --parent-lib /path/to/parent/libmpcmax.so [out.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops, utils, build, _lib as C  # noqa: E402
from motionpriorcmax_amd.utils.synth import synth_events  # noqa: E402

BLOCKS, STEPS, WARM = 9, 20, 10
dev = torch.device('cuda:0')
PARENT = None          # ctypes handle of the parent commit's library


def load_parent(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ('mpc_grid_traj_fwd', 'mpc_grid_traj_bwd', 'mpc_cvx_traj_fwd', 'mpc_cvx_traj_bwd', 'mpc_cvx_traj_bwd_workspace_bytes', 'mpc_version'):
        getattr(L, name).restype, getattr(L, name).argtypes = C.SIGNATURES[name]
    assert L.mpc_version() == 107
    return L


class ParentGridTrajFn(torch.autograd.Function):
    """ops.GridTrajFn for an fp32 grid and the polynomial basis, its two calls made into the parent commit's library."""

    @staticmethod
    def forward(ctx, cg, times, tile):
        B, S, c2, H, W = cg.shape
        k, n_t = c2 // 2, times.shape[0]
        traj = torch.empty((B, n_t, (H // tile) * (W // tile), 2), dtype=torch.float32, device=cg.device)
        rc = PARENT.mpc_grid_traj_fwd(ops._ptr(cg.detach()), ops._ptr(times), None, C.BASIS_POLY, 0.0, 1, ops._ptr(traj), None, B, S, k, H, W, tile, n_t,
                                      ops._stream(cg.device))
        assert rc == 0, rc
        ctx.save_for_backward(times)
        ctx.dims = (B, S, k, H, W, tile, n_t)
        return traj

    @staticmethod
    def backward(ctx, g):
        (times,) = ctx.saved_tensors
        B, S, k, H, W, tile, n_t = ctx.dims
        g = g.contiguous()
        gg = torch.empty((B, S, 2 * k, H, W), dtype=torch.float32, device=g.device)
        rc = PARENT.mpc_grid_traj_bwd(ops._ptr(g), ops._ptr(times), None, C.BASIS_POLY, 0.0, None, ops._ptr(gg), None, None, B, S, k, H, W, tile, n_t,
                                      ops._stream(g.device))
        assert rc == 0, rc
        return gg, None, None


class ParentCvxTrajFn(torch.autograd.Function):
    """ops.CvxCurveTrajFn for fp32 tensors (the mask's gradient alone), its calls made into the parent commit's library."""

    @staticmethod
    def forward(ctx, params, mask, bm, scale, tile):
        B, c2, h, w = params.shape
        d, T = c2 // 2, bm.shape[0]
        n = (8 * h // tile) * (8 * w // tile)
        traj = torch.empty((B, T, n, 2), dtype=torch.float32, device=params.device)
        p, m = params.detach(), mask.detach()
        rc = PARENT.mpc_cvx_traj_fwd(ops._ptr(p), ops._ptr(m), ops._ptr(bm), scale, ops._ptr(traj), B, d, T, h, w, tile, ops._stream(p.device))
        assert rc == 0, rc
        ctx.save_for_backward(p, m, bm)
        ctx.dims = (B, d, T, h, w, tile, scale)
        return traj

    @staticmethod
    def backward(ctx, g):
        p, m, bm = ctx.saved_tensors
        B, d, T, h, w, tile, scale = ctx.dims
        g = g.contiguous()
        gm = torch.empty((B, 576, h, w), dtype=torch.float32, device=g.device)
        rc = PARENT.mpc_cvx_traj_bwd(ops._ptr(g), ops._ptr(p), ops._ptr(m), ops._ptr(bm), scale, None, ops._ptr(gm), B, d, T, h, w, tile, None,
                                     ops._stream(g.device))
        assert rc == 0, rc
        return None, gm, None, None, None


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


def run_legs(legs):
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    samples = {m: [] for m in legs}
    for _ in range(BLOCKS):
        for m, fn in legs.items():
            samples[m].append(timed(fn))
    return {m: {'median_ms': round(statistics.median(v), 4), 'blocks_ms': [round(x, 4) for x in v]} for m, v in samples.items()}


def kernels_of(fn):
    with ops.KernelTimer() as kt:
        for _ in range(5):
            fn()
    return {k: {'launches_per_step': v['launches'] / 5, 'avg_us': round(v['avg_us'], 2)} for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}


def accept(r, native, base, f32, f32p):
    spread = max(max(r[m]['blocks_ms']) - min(r[m]['blocks_ms']) for m in (base, f32p) if m in r)
    out = {'spread_ms': round(spread, 4), 'native_minus_baseline_ms': round(r[native]['median_ms'] - r[base]['median_ms'], 4),
           'native_not_slower': r[native]['median_ms'] <= r[base]['median_ms'] + spread}
    if f32p in r:
        out['fp32_moved_ms'] = round(r[f32]['median_ms'] - r[f32p]['median_ms'], 4)
        out['fp32_unchanged'] = abs(r[f32]['median_ms'] - r[f32p]['median_ms']) <= spread
    return out


def grid_c3():
    wl = bench.WORKLOADS['C3']
    B, k, tile, H, W = 14, 3, bench.PATCH, bench.H, bench.W
    g = torch.Generator().manual_seed(3)
    x32 = torch.randn(B, 1, 2 * k, H, W, generator=g).to(dev)
    x16 = x32.to(torch.bfloat16).requires_grad_(True)
    x32.requires_grad_(True)
    times = torch.rand(16, generator=g).to(dev)
    go = torch.randn(B, 16, (H // tile) * (W // tile), 2, generator=g).to(dev)

    def node(x, up, parent):
        def run():
            xin = x.float() if up else x
            t = ParentGridTrajFn.apply(xin, times, tile) if parent else utils.trajectories_from_grid(xin, times, k, 'polynomial', tile)[0]
            t.backward(go)
            assert x.grad.dtype == x.dtype
            x.grad = None
        return run

    ev, npos = synth_events(B, wl['M'], (H, W), wl['nb'], seed=1, pad_frac=0.02, time_sorted=True)
    batch = {'events': ev.to(dev), 'num_pos_events': npos}
    L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))

    def step(x, up, parent):
        def run():
            tm = L.get_reconstruction_times(dev)
            xin = x.float() if up else x
            t = ParentGridTrajFn.apply(xin, tm, tile) if parent else utils.trajectories_from_grid(xin, tm, k, 'polynomial', tile)[0]
            loss, _, _ = L.calc(t, tm, batch)
            loss.backward()
            x.grad = None
        return run

    legs = {'native': node(x16, False, False), 'upcast': node(x16, True, False), 'fp32': node(x32, False, False),
            'step_native': step(x16, False, False), 'step_upcast': step(x16, True, False)}
    if PARENT is not None:
        legs.update({'upcast_parent': node(x16, True, True), 'fp32_parent': node(x32, False, True), 'step_upcast_parent': step(x16, True, True)})
    r = run_legs(legs)
    r['kernels'] = {m: kernels_of(legs[m]) for m in ('native', 'upcast')}
    base = 'upcast_parent' if PARENT is not None else 'upcast'
    r['accept_node'] = accept(r, 'native', base, 'fp32', 'fp32_parent')
    r['accept_step'] = accept(r, 'step_native', 'step_' + base, 'fp32', 'fp32_parent')
    n = x32.numel()
    r['shape'] = dict(grid=[B, 1, 2 * k, H, W], k=k, basis='polynomial', tile=tile, n_t=16, dtype='bfloat16', M=wl['M'])
    r['bytes_removed_from_shapes'] = dict(float_copy_read_write=2 * n + 4 * n, grad_cast_read_write=4 * n + 2 * n, grad_write_saved=2 * n,
                                          total=14 * n)
    return r


def head_c4():
    B, d, h, w, tile, T = 6, 10, 48, 64, 4, 42
    g = torch.Generator().manual_seed(4)
    params = (torch.randn(B, 2 * d, h, w, generator=g) * 0.5).to(dev)
    m32 = torch.randn(B, 576, h, w, generator=g).to(dev)
    m16 = m32.to(torch.bfloat16).requires_grad_(True)
    m32.requires_grad_(True)
    bm = utils.bernstein_basis(torch.linspace(0, 1, T).numpy(), d).to(dev)
    go = torch.randn(B, T, (8 * h // tile) * (8 * w // tile), 2, generator=g).to(dev)

    def node(m, up, parent):
        def run():
            mi = m.float() if up else m
            t = ParentCvxTrajFn.apply(params, mi, bm, 1.0, tile) if parent else ops.CvxCurveTrajFn.apply(params, mi, bm, 1.0, tile)
            t.backward(go)
            assert m.grad.dtype == m.dtype
            m.grad = None
        return run

    legs = {'native': node(m16, False, False), 'upcast': node(m16, True, False), 'fp32': node(m32, False, False)}
    if PARENT is not None:
        legs.update({'upcast_parent': node(m16, True, True), 'fp32_parent': node(m32, False, True)})
    r = run_legs(legs)
    r['kernels'] = {m: kernels_of(legs[m]) for m in ('native', 'upcast')}
    r['accept_node'] = accept(r, 'native', 'upcast_parent' if PARENT is not None else 'upcast', 'fp32', 'fp32_parent')
    n = m32.numel()
    r['shape'] = dict(params=[B, 2 * d, h, w], mask=[B, 576, h, w], tile=tile, n_t=T, dtype='bfloat16', gradient='the mask alone')
    r['bytes_removed_from_shapes'] = dict(float_copy_read_write=6 * n, grad_cast_read_write=6 * n, grad_write_saved=2 * n, total=14 * n)
    return r


def main():
    global PARENT
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'half_heads.json'))
    a = ap.parse_args()
    if a.parent_lib:
        PARENT = load_parent(a.parent_lib)
    res = {'source_hash': build.source_hash(), 'parent_library': bool(a.parent_lib),
           'method': f'one process, legs alternating inside each of {BLOCKS} blocks; a block: {STEPS} steps between two device events after {WARM} warm-up '
                     'steps; a leg: the median over its blocks; spread: max - min over the blocks of the parent legs (of `upcast` without a parent library)',
           'workloads': {}}
    for name, fn in (('C3_grid', grid_c3), ('C4_head', head_c4)):
        r = res['workloads'][name] = fn()
        print(name, json.dumps({m: v['median_ms'] for m, v in r.items() if isinstance(v, dict) and 'median_ms' in v}),
              json.dumps({k: v for k, v in r.items() if k.startswith('accept')}), flush=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
