#!/usr/bin/env python3
"""utils.ingest_raw_events(dataset='evimo2') (csrc/ingest.hip, the window kernels) against a plain-torch mirror of the op chain the
reference runs per sample in its DataLoader workers (mask, normalise, searchsorted, split; then pad and stack), both on the same GPU
tensors in ONE process, alternating call by call: median of CALLS calls after warm-up, host clock around a call that ends in a device
synchronise.  bench.py's C4 and C4b6 shapes: B = 1 and B = 6, windows of ~1.2 M events (0.4 s of context + 0.3 s) of which ~500k
are kept, 41 bins, int32 coordinates, int64 polarity, as the EVIMO2 loader produces them.
Per-kernel times from ops.KernelTimer and the bytes the kept suffix needs (28 B read per kept event, 24 B written per output row).
Writes profiles/ingest_window.json (tagged with build.source_hash()):
    python tools/ingest_window_probe.py [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import build, ops  # noqa: E402
from motionpriorcmax_amd.utils import ingest_raw_events  # noqa: E402

CALLS, WARM = 25, 5
NB, DURATION_MS, N_WINDOW = 41, 300, 1_200_000
dev = torch.device('cuda:0')


def synth(B, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    counts = [N_WINDOW - 37_001 * b for b in range(B)]
    N = max(counts)
    x = torch.randint(0, 640, (B, N), generator=g, device=dev, dtype=torch.int32)
    y = torch.randint(0, 480, (B, N), generator=g, device=dev, dtype=torch.int32)
    p = torch.randint(0, 2, (B, N), generator=g, device=dev, dtype=torch.int64)
    t = torch.zeros((B, N), dtype=torch.int64, device=dev)
    for b, n in enumerate(counts):
        t[b, :n] = 100_000_000 + 50_000 * b + torch.sort(torch.randint(0, 700_000, (n,), generator=g, device=dev)).values
    return x, y, t, p, counts


def mirror(x, y, t, p, counts, edges):
    """The per-sample chain in torch's own promotion rules (int64 stamp minus a Python float -> fp32), then the collate."""
    pos, neg = [], []
    for b, n in enumerate(counts):
        ts = t[b, :n]
        rows = torch.stack((y[b, :n].long(), x[b, :n].long(), ts, p[b, :n]), dim=1)
        start = ts[-1] - DURATION_MS * 1e3
        ev = rows[rows[:, 2] > start].float()
        ev[:, 2] = (ev[:, 2] - start) / (ts[-1] - start)
        bins = torch.searchsorted(edges, ev[:, 2].contiguous()) - 1
        bins[bins == -1] = 0
        ev = torch.cat((ev, bins[:, None]), dim=1)
        pos.append(ev[ev[:, 3] == 1])
        neg.append(ev[ev[:, 3] == 0])
    mp, mn = max(len(e) for e in pos), max(len(e) for e in neg)          # (a host read, as the library's two maxima)
    out = torch.zeros((len(counts), mp + mn, 6), dtype=torch.float32, device=dev)
    for b, (a, c) in enumerate(zip(pos, neg)):
        out[b, :len(a), :5] = a
        out[b, :len(a), 5] = 1
        out[b, mp:mp + len(c), :5] = c
        out[b, mp:mp + len(c), 5] = 1
    return out, mp


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main(out):
    if not torch.cuda.is_available():
        raise SystemExit('this probe measures on the GPU; there is none here')
    res = {'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(dev), 'calls': CALLS, 'warmup': WARM,
           'num_bins': NB, 'flow_duration_ms': DURATION_MS, 'timing': 'host clock around one call ending in a device synchronise; '
           'library and mirror alternate call by call', 'batches': {}}
    edges = torch.linspace(0, 1, NB + 1).to(dev)
    for B in (1, 6):
        x, y, t, p, counts = synth(B, seed=20 + B)
        cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        lib = lambda: ingest_raw_events(x, y, t, p, cnt, NB, 'evimo2', flow_duration_ms=DURATION_MS)
        mir = lambda: mirror(x, y, t, p, counts, edges)
        a, (m_ev, m_pos) = lib(), mir()
        same = bool(a['num_pos_events'] == m_pos and torch.equal(a['events'], m_ev))
        kept = int(a['events'][..., 5].sum().item())
        for _ in range(WARM):
            lib(); mir()
        s_lib, s_mir = [], []
        for _ in range(CALLS):
            s_lib.append(timed(lib)); s_mir.append(timed(mir))
        with ops.KernelTimer() as kt:
            for _ in range(5):
                lib()
        kern = {k: {'launches_per_call': v['launches'] / 5, 'avg_us': round(v['avg_us'], 2)}
                for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
        kernel_us = sum(v['avg_us'] * v['launches_per_call'] for v in kern.values())
        # x, y, t, p of the kept suffix (24 B) + 4 B for the count pass, every row written once.  (The count pass re-reads the
        # 8-byte polarity, so the traffic is understated by 4 B per kept event.)
        need = kept * (4 + 4 + 8 + 8 + 4) + int(a['events'].numel()) * 4
        ml, mm = statistics.median(s_lib), statistics.median(s_mir)
        r = {'workload': dict(B=B, window_events=counts, kept_events=kept, rows_per_sample=int(a['events'].shape[1])),
             'library_ms': {'median': round(ml, 4), 'min': round(min(s_lib), 4), 'max': round(max(s_lib), 4)},
             'mirror_ms': {'median': round(mm, 4), 'min': round(min(s_mir), 4), 'max': round(max(s_mir), 4)},
             'mirror_over_library': round(mm / ml, 2), 'library_not_slower': bool(ml <= mm),
             'library_equals_mirror_bitwise': same, 'kernels': kern, 'kernel_us_per_call': round(kernel_us, 1),
             'needed_bytes': need, 'achieved_GBps_over_kernel_time': round(need / kernel_us / 1e3, 1) if kernel_us else None}
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps(r), flush=True)
    res['library_not_slower_at_both_shapes'] = all(r['library_not_slower'] for r in res['batches'].values())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'ingest_window.json'))
