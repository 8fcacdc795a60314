#!/usr/bin/env python3
"""The EVIMO2 network input at the C4 batch (B = 6, 65 x 480 x 640 -> normalised -> 384 x 512), in ONE process,
the call and its comparators alternating: median of 7 blocks of 10 calls after warm-up, host clock ending in a device
synchronise, input batches rotated (three batches of 180 MB at 1 500 000 events per sample: more than the Infinity Cache).
  lib_fused     utils.representation_grids(normalize=True, out_size=(384, 512)): the resize inside the write pass
  lib_unfused   the same call without out_size (full-size normalised grid), then F.interpolate on the device
  torch_ops     the comparator that is not the code under test: the seven steps with torch operators on the device
                (index_put_(accumulate=True), masked mean / std, F.interpolate) -- what a user has without this library
  dsec_voxel    the existing DSEC builder utils.voxel_grids on the same events at 15 channels (its records and strips are the same
                machinery: a sanity row for the binning and accumulate rates)
Synthetic events from oracle.repr_oracle.synth_int_events (the real count per EVIMO2 window is not known here), rows at
1 500 000 and 500 000 events per sample.  Per-kernel times from the library's own events (mpc_profile_start / _stop) in a pass
of their own after the timed blocks.  Writes profiles/repr_grid.json (tagged with build.source_hash()):
    python tools/repr_probe.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from motionpriorcmax_amd import _lib as C, build, utils  # noqa: E402
from oracle import repr_oracle as R  # noqa: E402

BLOCKS, STEPS, WARM, ROTATE = 7, 10, 3, 3
B, CH, H, W, OUT = 6, 65, 480, 640, (384, 512)
T_LO, T_HI = 41234567, 41534567            # a 300 ms window in absolute microseconds
HBM = 8.0e12
dev = torch.device('cuda:0')


def torch_ops(x, y, p, t, counts):
    """Steps 1-7 with torch operators, batched, no host synchronisation."""
    Bn, N = x.shape
    valid = torch.arange(N, device=dev)[None] < counts[:, None]
    c0 = t[:, :1]
    c1 = t.gather(1, (counts.long() - 1).clamp(min=0)[:, None])
    tn = (t - c0).float() / (c1 - c0).float() * float(CH - 1)
    t0 = tn.floor().long()
    val = 2 * p - 1
    base = (torch.arange(Bn, device=dev)[:, None] * CH * H * W + y.long() * W + x.long())
    grid = torch.zeros(Bn * CH * H * W, device=dev)
    for tl in (t0, t0 + 1):
        m = valid & (tl >= 0) & (tl < CH)                       # a masked-out vote adds 0 to entry 0: no boolean indexing, no host sync
        w = torch.where(m, val * (1 - (tl.float() - tn).abs()), 0.0)
        grid.index_put_((torch.where(m, base + tl * (H * W), 0).view(-1),), w.view(-1), accumulate=True)
    grid = grid.view(Bn, CH, H, W)
    nz = grid != 0
    n = nz.sum((1, 2, 3), keepdim=True).float()
    mean = grid.sum((1, 2, 3), keepdim=True) / n.clamp(min=1)
    var = (((grid - mean) ** 2) * nz).sum((1, 2, 3), keepdim=True) / (n - 1)
    std = var.sqrt()
    normed = torch.where(nz, torch.where(std > 0, (grid - mean) / std, grid - mean), grid)
    return F.interpolate(normed, size=OUT, mode='bilinear', align_corners=False)


def kernel_times(fn, reps=5):
    """Mean duration of every kernel launch of the library inside fn(), full kernel names (template arguments kept)."""
    L = C.lib()
    torch.cuda.synchronize()
    L.mpc_profile_start()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    cap = 1 << 12
    names = ctypes.create_string_buffer(cap * 48)
    ms = (ctypes.c_float * cap)()
    n = int(L.mpc_profile_stop(names, len(names), ms, cap))
    out = {}
    for nm, v in zip(names.value.decode().split('\n')[:n], ms[:n]):
        r = out.setdefault(nm.strip().strip('()'), [0, 0.0])
        r[0] += 1
        r[1] += 1e3 * v
    return {k: {'launches_per_call': c / reps, 'avg_us': round(tot / c, 2)} for k, (c, tot) in out.items()}


def main(out):
    res = {'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(0),
           'method': f'one process, modes alternating, median of {BLOCKS} blocks x {STEPS} calls after {WARM} warm-up calls per mode; host clock '
                     f'ending in torch.cuda.synchronize(); {ROTATE} input batches rotated; per-kernel: mpc_profile_start/_stop in a pass of its own',
           'shape': dict(B=B, channels=CH, height=H, width=W, out_size=list(OUT), normalize=True, centres='default (first / last event)'),
           'rows': {}}
    for n_ev in (1500000, 500000):
        batches = []
        for r in range(ROTATE):
            s = [R.synth_int_events(n_ev, (CH, H, W), T_LO, T_HI, 100 + 10 * r + b) for b in range(B)]
            x = torch.stack([v[0] for v in s]).float().to(dev)
            y = torch.stack([v[1] for v in s]).float().to(dev)
            p = torch.stack([v[2] for v in s]).float().to(dev)
            t = torch.stack([v[3] for v in s]).to(dev)
            cnt = torch.full((B,), n_ev, dtype=torch.int32, device=dev)
            xytp = torch.stack((x, y, (t - t[:, :1]).float(), p), -1).contiguous()
            batches.append(dict(x=x, y=y, p=p, t=t, cnt=cnt, xytp=xytp))
        it = [0]

        def nxt():
            it[0] += 1
            return batches[it[0] % ROTATE]

        def lib_call(d, out_size):
            # the ABI's dtypes (fp32 x, y, pol, int64 time): passed through without a conversion pass; int_xy=True selects the two-tap path
            return utils.representation_grids(d['x'], d['y'], d['p'], d['t'], d['cnt'], CH, H, W, normalize=True, out_size=out_size, int_xy=True)

        modes = {
            'lib_fused': lambda: lib_call(nxt(), OUT),
            'lib_unfused': lambda: F.interpolate(lib_call(nxt(), None), size=OUT, mode='bilinear', align_corners=False),
            'torch_ops': lambda: (lambda d: torch_ops(d['x'], d['y'], d['p'], d['t'], d['cnt']))(nxt()),
            'dsec_voxel': lambda: (lambda d: utils.voxel_grids(d['xytp'], d['cnt'], (15, H, W), 'mean_std'))(nxt()),
        }
        # the comparator computes the same thing (fp32 atomics in another order: last bits)
        d = batches[0]
        a, b_ = lib_call(d, OUT), torch_ops(d['x'], d['y'], d['p'], d['t'], d['cnt'])
        u = F.interpolate(lib_call(d, None), size=OUT, mode='bilinear', align_corners=False)
        agree = dict(fused_vs_torch_ops_max_abs=float((a - b_).abs().max()), fused_vs_unfused_max_abs=float((a - u).abs().max()),
                     out_abs_max=float(a.abs().max()))
        del a, b_, u
        for fn in modes.values():
            for _ in range(WARM):
                fn()
        samples = {m: [] for m in modes}
        for _ in range(BLOCKS):
            for m, fn in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    fn()
                torch.cuda.synchronize()
                samples[m].append(1e3 * (time.perf_counter() - t0) / STEPS)
        row = {m: {'median_ms': round(statistics.median(v), 4), 'blocks_ms': [round(q, 4) for q in v]} for m, v in samples.items()}
        for m in ('lib_fused', 'lib_unfused', 'torch_ops'):
            row[m]['events_per_s'] = round(B * n_ev / (row[m]['median_ms'] * 1e-3))
        alg = 20 * B * n_ev + 4 * B * CH * OUT[0] * OUT[1]
        row['algorithmic_bytes'] = alg
        row['lib_fused']['fraction_of_8TBps'] = round(alg / (row['lib_fused']['median_ms'] * 1e-3) / HBM, 4)
        row['speedup_vs_torch_ops'] = round(row['torch_ops']['median_ms'] / row['lib_fused']['median_ms'], 2)
        row['fused_over_unfused'] = round(row['lib_fused']['median_ms'] / row['lib_unfused']['median_ms'], 3)
        row['agreement'] = agree
        row['kernels'] = {'lib_fused': kernel_times(modes['lib_fused']), 'lib_unfused': kernel_times(lambda: lib_call(nxt(), None)),
                          'dsec_voxel': kernel_times(modes['dsec_voxel'])}
        res['rows'][str(n_ev)] = row
        print(n_ev, json.dumps({m: row[m]['median_ms'] for m in modes}), json.dumps(row['kernels']['lib_fused']), json.dumps(agree), flush=True)
        del batches, modes
        torch.cuda.empty_cache()
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'repr_grid.json'))
