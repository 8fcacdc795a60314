"""The fused IWE pyramid pass (csrc/iwe_pyramid.hip) against the stage-call route it replaces: one MI355X, one process, this tree's
library and -- with --parent-lib -- the parent commit's library loaded beside it, the legs alternated round by round.
-> profiles/iwe_pyramid.json (or the path given).

  calc      the C3 step (forward + backward) at pyramid_levels 1 and 3 on white-noise events (bench.synth_inputs) and on the same
            batch bucket-ordered (FocusLoss.order_events); levels = 3 on the fused pass and on the stage calls (pyramid_fused=False);
            with a parent library the levels = 1 step and the stage-call levels = 3 step once more through that library
  per_event calc_per_event_basis at the DSEC batch shape (C3: k = 3) and calc_per_event_curves at C4 (Bezier d = 10, up_mask), both
            bucket-ordered, at levels 1 and 3
  kernels   per-kernel HIP events (ops.KernelTimer) of the fused and of the stage-call levels = 3 step and of the staged levels = 1
            step: the three new launches, and the pooling / contrast / finalize launches of the coarse levels they replace
  memory    peak allocated bytes of forward + backward per leg
  conditions (i) pyramid3_C3: stage calls (the parent's route; through the parent's library where given) minus fused > the larger
            spread of the two legs; (ii) the three new launches <= the coarse levels' k_pool2_* + k_contrast_march + k_finalize;
            (iii) the levels = 1 step unchanged within spread; (iv) peak memory at levels = 3 not above the stage-call route's.

    python tools/iwe_pyramid_probe.py [--parent-lib /path/to/parent/libmpcmax.so] [--rounds 5] [out.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from motionpriorcmax_amd import LossFactory, _lib as C, build, ops

DEV = torch.device('cuda:0')
STEPS = 10


def load_parent(path):
    """The parent commit's library with the binding's signatures on every symbol it has (it lacks the pass's three)."""
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
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def run_legs(legs, rounds):
    """legs {name: (library handle or None, step)} alternated round by round -> {name: ms per step: median, min, max, spread; peak bytes}."""
    out = {}
    for name, (h, fn) in legs.items():
        with using(h):
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            out[name] = {'ms': [], 'peak_bytes_above_inputs': int(torch.cuda.max_memory_allocated() - base)}
    for _ in range(rounds):
        for name, (h, fn) in legs.items():
            with using(h):
                out[name]['ms'].append(timed(fn))
    for r in out.values():
        ms = sorted(r.pop('ms'))
        r.update(ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), spread_ms=round(ms[-1] - ms[0], 4))
    return out


def kernel_table(h, fn):
    with using(h):
        fn()
        with ops.KernelTimer() as kt:
            for _ in range(STEPS):
                fn()
    return {k: {'us_per_step': round(v['total_us'] / STEPS, 2), 'launches_per_step': v['launches'] / STEPS} for k, v in
            sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}


def calc_step(L, traj, times, batch):
    def step():
        loss, _, _ = L.calc(traj, times, batch)
        loss.backward()
        traj.grad = None
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('out', nargs='?', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'iwe_pyramid.json'))
    a = ap.parse_args()
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    res = {'source_hash': build.source_hash(), 'parent_library': bool(a.parent_lib), 'device': torch.cuda.get_device_name(0),
           'steps_per_timing': STEPS, 'rounds': a.rounds}

    # ---- calc, C3 -------------------------------------------------------------------------------------------------------------
    wl = bench.WORKLOADS['C3']
    ev, npos, tr, tm = bench.synth_inputs(wl, seed=1)
    cfg = dict(bench.loss_config(wl), auto_static_shapes=False)
    L1 = LossFactory.get_loss_calculator('FOCUS', cfg)
    L3 = LossFactory.get_loss_calculator('FOCUS', dict(cfg, pyramid_levels=3))
    L3s = LossFactory.get_loss_calculator('FOCUS', dict(cfg, pyramid_levels=3, pyramid_fused=False))
    traj, times = tr.to(DEV).requires_grad_(True), tm.to(DEV)
    white = {'events': ev.to(DEV), 'num_pos_events': npos}
    ordered = L1.order_events(white)
    legs = {'levels1_white': (None, calc_step(L1, traj, times, white)), 'levels3_fused_white': (None, calc_step(L3, traj, times, white)),
            'levels3_stage_white': (None, calc_step(L3s, traj, times, white)),
            'levels1_ordered': (None, calc_step(L1, traj, times, ordered)), 'levels3_fused_ordered': (None, calc_step(L3, traj, times, ordered))}
    if parent is not None:
        legs['parent_levels1_white'] = (parent, calc_step(L1, traj, times, white))
        legs['parent_levels3_stage_white'] = (parent, calc_step(L3s, traj, times, white))
        legs['parent_levels1_ordered'] = (parent, calc_step(L1, traj, times, ordered))
    res['calc_C3'] = run_legs(legs, a.rounds)
    # the two routes state the same loss
    with torch.no_grad():
        lf, ls = L3.calc(traj, times, white)[0], L3s.calc(traj, times, white)[0]
    res['calc_C3']['loss_fused_vs_stage'] = [float(lf), float(ls)]

    # ---- per-kernel times -----------------------------------------------------------------------------------------------------
    kt = {'levels3_fused': kernel_table(None, legs['levels3_fused_white'][1])}
    sh, sfn = (parent, legs['parent_levels3_stage_white'][1]) if parent is not None else (None, legs['levels3_stage_white'][1])
    kt['levels3_stage'] = kernel_table(sh, sfn)
    ops.FUSED_CALLS = False          # (the staged levels = 1 step: the same stage calls without the coarse levels)
    try:
        kt['levels1_staged'] = kernel_table(sh, legs['levels1_white'][1])
    finally:
        ops.FUSED_CALLS = True
    new_us = sum(kt['levels3_fused'].get(k, {}).get('us_per_step', 0.0) for k in ('k_iwe_pyramid_levels', 'k_iwe_pyramid_reduce', 'k_iwe_pyramid_fold'))
    old = ('k_pool2_fwd', 'k_pool2_bwd_add', 'k_contrast_march', 'k_finalize')
    old_us = sum(kt['levels3_stage'].get(k, {}).get('us_per_step', 0.0) - kt['levels1_staged'].get(k, {}).get('us_per_step', 0.0) for k in old)
    res['kernels'] = dict(kt, new_launches_us=round(new_us, 2), replaced_launches_us=round(old_us, 2))

    # ---- per-event routes -----------------------------------------------------------------------------------------------------
    del legs
    g = torch.Generator().manual_seed(8)
    coeff = (torch.randn(wl['B'], 1, 2 * wl['k'], bench.H, bench.W, generator=g)).to(DEV).requires_grad_(True)

    def basis_step(L):
        def step():
            loss, _, _ = L.calc_per_event_basis(coeff, 0.41, ordered, wl['k'])
            loss.backward()
            coeff.grad = None
        return step
    pe = run_legs({'basis_C3_levels1': (None, basis_step(L1)), 'basis_C3_levels3': (None, basis_step(L3))}, a.rounds)
    del coeff, white, ordered, traj
    wl4 = bench.WORKLOADS['C4']
    from motionpriorcmax_amd.utils.synth import synth_events
    ev4, np4 = synth_events(1, wl4['M'], (bench.H, bench.W), wl4['nb'], seed=1, pad_frac=0.02, time_sorted=True)
    cfg4 = dict(bench.loss_config(wl4), auto_static_shapes=False)
    C1 = LossFactory.get_loss_calculator('FOCUS', cfg4)
    C3_ = LossFactory.get_loss_calculator('FOCUS', dict(cfg4, pyramid_levels=3))
    b4 = C1.order_events({'events': ev4.to(DEV), 'num_pos_events': np4})
    params = (torch.randn(1, 20, bench.H // 8, bench.W // 8, generator=g) * 0.25).to(DEV).requires_grad_(True)
    mask = torch.randn(1, 576, bench.H // 8, bench.W // 8, generator=g).to(DEV).requires_grad_(True)

    def curves_step(L):
        def step():
            loss, _, _ = L.calc_per_event_curves(params, 0.41, b4, up_mask=mask, curve_type='BEZIER')
            loss.backward()
            params.grad = mask.grad = None
        return step
    pe.update(run_legs({'curves_C4_levels1': (None, curves_step(C1)), 'curves_C4_levels3': (None, curves_step(C3_))}, a.rounds))
    res['per_event'] = pe

    # ---- conditions -----------------------------------------------------------------------------------------------------------
    c = res['calc_C3']
    stage = c['parent_levels3_stage_white'] if parent is not None else c['levels3_stage_white']
    fused = c['levels3_fused_white']
    gain = stage['ms_median'] - fused['ms_median']
    cond = {'i_pyramid3_C3_drops': dict(stage_ms=stage['ms_median'], fused_ms=fused['ms_median'], gain_ms=round(gain, 4),
                                        spread_ms=max(stage['spread_ms'], fused['spread_ms']), met=bool(gain > max(stage['spread_ms'], fused['spread_ms']))),
            'ii_new_launches_cost_no_more': dict(new_us=res['kernels']['new_launches_us'], replaced_us=res['kernels']['replaced_launches_us'],
                                                 met=bool(new_us <= old_us)),
            'iv_peak_memory': dict(fused_bytes=fused['peak_bytes_above_inputs'], stage_bytes=stage['peak_bytes_above_inputs'],
                                   met=bool(fused['peak_bytes_above_inputs'] <= stage['peak_bytes_above_inputs']))}
    if parent is not None:
        for k in ('white', 'ordered'):
            p1, t1 = c[f'parent_levels1_{k}'], c[f'levels1_{k}']
            gap = t1['ms_median'] - p1['ms_median']
            cond[f'iii_levels1_unchanged_{k}'] = dict(parent_ms=p1['ms_median'], tree_ms=t1['ms_median'], gap_ms=round(gap, 4),
                                                      spread_ms=max(p1['spread_ms'], t1['spread_ms']), met=bool(gap <= max(p1['spread_ms'], t1['spread_ms'])))
    res['conditions'] = cond
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res['conditions'], indent=1))
    print(json.dumps({k: v for k, v in res['calc_C3'].items()}, indent=1))
    print(json.dumps(res['per_event'], indent=1))
    print(json.dumps({k: res['kernels'][k] for k in ('new_launches_us', 'replaced_launches_us')}))


if __name__ == '__main__':
    main()
