#!/usr/bin/env python3
"""Step and per-kernel times of the per-event warp with a TABULATED basis (FocusLoss.calc_per_event_basis(basis_type='table'))
against the routes it stands beside, at the per-event row of bench.py (C3: 14 x 200 k events, 480 x 640, k = 3), on a time-sorted
batch (the loader's) and on a bucket-ordered one:

    1 polynomial   the fused node, basis worked out in the kernels (the no-regression control)
    2 learned      the reference's MLP 1 -> 64 -> 64 -> 64 -> 3 evaluated at EVERY event, its values constants (no basis gradient)
    3 table        S = 1024 knots from the same MLP (utils.basis_table), the basis gradient included: the MLP's backward at the knots
    4 mirror       plain torch: the MLP inside the graph at every event (what training it without a table costs); peak memory too

Median of 25 steps per route, the routes ALTERNATING inside every round of one process (so that clock and temperature drift hit
all of them alike), every step timed from the host with a device synchronisation on both sides; then the per-kernel times of 5
steps from ops.KernelTimer.  Routes 3 and 4 exist from the commit that adds the table on; on an older checkout the probe times
routes 1 and 2 and says so.  `--merge FILE`: figures of another run (a parent checkout's) to put into the output as "parent".
`--control`: routes 1 and 2 only on any checkout -- the no-regression comparison wants the SAME process on both sides (a step that
follows the 29 ms mirror step of route 4 starts from other clocks and another allocator state than one that follows a 3 ms step).

    python tools/pe_table_probe.py [--out profiles/pe_table.json] [--merge parent.json] [--steps 25]

Also reports how well S = 1024 represents the reference's trained basis network (golden g11_learned_basis): the maximum of
|table_basis_values(T, t) - net(t)| over 10^5 times."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import bench  # noqa: E402
from motionpriorcmax_amd import LossFactory, ops, utils  # noqa: E402
from motionpriorcmax_amd.build import source_hash  # noqa: E402


def mlp(k, dev):
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(),
                         nn.Linear(64, k)).to(dev)


def mirror_step(L, cg, net, t_ref, batch, k):
    """calc_per_event_basis(fused=False) with the network INSIDE the graph: phi [B, M, k] from the MLP at every event."""
    ev = batch['events']
    B, M = ev.shape[0], ev.shape[1]
    hq, wq = L._cfg.lut_grid
    sp = L.lut_superpixel_size
    tr = torch.full((1,), float(t_ref), device=ev.device)
    phi = net(tr[:, None]) - net(ev[..., 2:3])
    c_rows = ops.TileCoeffRowsFn.apply(cg, sp)
    with torch.no_grad():
        iy = torch.div(ev[..., 0], sp, rounding_mode='floor').long().clamp_(0, hq - 1)
        ix = torch.div(ev[..., 1], sp, rounding_mode='floor').long().clamp_(0, wq - 1)
        idx = (torch.arange(B, device=ev.device).view(-1, 1) * hq * wq + iy * wq + ix).reshape(-1)
    ce = ops.GatherRowsFn.apply(c_rows, idx).view(B, M, 2, k)
    warped = ev[..., :2] + (ce * phi[:, :, None, :]).sum(-1)
    focus, _ = ops.PrewarpedFocusFn.apply(warped, ev, tr, L._cfg, int(batch['num_pos_events']))
    tm = utils.synth.bin_mid_times(L.num_bins).to(ev.device)
    phim = net(tr[:, None]) - net(tm[:, None])
    field = (c_rows.reshape(B * hq * wq * 2, k) @ phim.t()).view(B, hq * wq, 2, L.num_bins).permute(0, 3, 1, 2).reshape(B * L.num_bins, hq, wq, 2)
    return focus + ops.LutSmoothFn.apply(field, L._cfg, float(L.smooth_weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pe_table.json'))
    ap.add_argument('--merge', default=None)
    ap.add_argument('--steps', type=int, default=25)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--control', action='store_true', help='routes 1 and 2 only: the same process on either side of a parent / new comparison')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    wl = bench.WORKLOADS['C3']
    k = wl['k']
    have_table = hasattr(utils, 'basis_table') and not args.control
    ev, npos, _, _ = bench.synth_inputs(wl, seed=1)            # (time-sorted inside the polarity blocks, as the loader delivers)
    L = LossFactory.get_loss_calculator('FOCUS', bench.loss_config(wl))
    g = torch.Generator().manual_seed(8)
    cg = torch.randn(wl['B'], 1, 2 * k, bench.H, bench.W, generator=g).to(dev).requires_grad_(True)
    net = mlp(k, dev)
    sorted_b = {'events': ev.to(dev), 'num_pos_events': npos}
    batches = {'time_sorted': sorted_b, 'bucket_ordered': L.order_events(sorted_b)}
    result = {'workload': 'C3 per-event row: B=14, M=200000, 480x640, k=3, nb=15', 'samples': args.samples, 'steps': args.steps,
              'source_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'has_table_route': have_table, 'layouts': {}}

    def clear():
        cg.grad = None
        for p in net.parameters():
            p.grad = None

    for lname, b in batches.items():
        def r_poly():
            loss, _, _ = L.calc_per_event_basis(cg, 0.41, b, k)
            loss.backward()

        def r_learned():
            loss, _, _ = L.calc_per_event_basis(cg, 0.41, b, k, 'learned', net)
            loss.backward()

        def r_table():
            T = utils.basis_table('learned', k, args.samples, net)
            loss, _, _ = L.calc_per_event_basis(cg, 0.41, b, k, 'table', basis_table=T)
            loss.backward()

        def r_mirror():
            mirror_step(L, cg, net, 0.41, b, k).backward()
        routes = {'polynomial': r_poly, 'learned_constants': r_learned}
        if have_table:
            routes['table'] = r_table
            routes['torch_mirror_trains_mlp'] = r_mirror
        times = {n: [] for n in routes}
        for n, fn in routes.items():
            for _ in range(3):
                fn()
                clear()
        torch.cuda.synchronize()
        for _ in range(args.steps):
            for n, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[n].append(1e3 * (time.perf_counter() - t0))
                clear()
        out = {}
        for n, fn in routes.items():
            with ops.KernelTimer() as kt:
                for _ in range(5):
                    fn()
                    clear()
            ks = {kn: round(v['total_us'] / 5, 1) for kn, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
            ts = sorted(times[n])
            out[n] = {'median_ms': round(statistics.median(ts), 4), 'min_ms': round(ts[0], 4), 'p90_ms': round(ts[int(0.9 * (len(ts) - 1))], 4),
                      'library_kernels_us_per_step': ks, 'library_kernels_total_us': round(sum(ks.values()), 1)}
            print(f'{lname} {n}: median {out[n]["median_ms"]} ms (min {out[n]["min_ms"]}, p90 {out[n]["p90_ms"]}); library kernels '
                  f'{out[n]["library_kernels_total_us"]} us: ' + ' '.join(f'{a}={v}' for a, v in list(ks.items())[:8]), flush=True)
        if have_table:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r_mirror()
            torch.cuda.synchronize()
            out['torch_mirror_trains_mlp']['peak_allocated_MB_above_inputs'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            clear()
            torch.cuda.reset_peak_memory_stats()
            r_table()
            torch.cuda.synchronize()
            out['table']['peak_allocated_MB_above_inputs'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            clear()
        result['layouts'][lname] = out
    if have_table:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'g11_learned_basis.npz'), allow_pickle=False)
        gnet = nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(),
                             nn.Linear(64, int(z['num_basis'])))
        gnet.load_state_dict({kk: torch.from_numpy(z['net_' + kk.replace('.', '_')]) for kk in gnet.state_dict()})
        t = torch.rand(100_000, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        fid = {}
        with torch.no_grad():
            ref = gnet.double()(t[:, None])
            for S in (64, 256, 1024, 4096):
                T = utils.basis_table('learned', int(z['num_basis']), S, gnet.float())
                fid[str(S)] = float((utils.table_basis_values(T, t.float()).double() - ref).abs().max())
                gnet.double()
            fid['max_abs_basis'] = float(ref.abs().max())
        result['table_fidelity_g11_learned_basis_max_abs_error'] = fid
        print('fidelity of the table to the g11 network (max |error| over 1e5 times):', fid)
    if args.merge:
        result['parent'] = json.load(open(args.merge))
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
