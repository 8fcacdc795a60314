#!/usr/bin/env python3
"""The three DSEC steps that moved to the device, each timed beside what a caller of the commit before them would run on the
device for the same result, in ONE process, alternating call by call (the discipline of tools/flow_targets_probe.py: HIP events
around every call, median of CALLS calls after WARM warm-up calls, every call on another buffer of a pool larger than the 256 MB
Infinity Cache, and a plain device-to-device copy of the same number of bytes as the streaming yardstick):

  A  ingest_events(rectify_map=m)                 vs  torch gather m[y, x] (+ two .contiguous()) + ingest_events on the floats
     14 x 200 000 events, 480 x 640 map, with the (x, y, t, p) rows for the voxel grid; plain layout and bucket order
  B  dsec_flow_error(png16, pred)                 vs  torch decode of the payload + calculate_flow_error
     dsec_flow_targets(png16)                     vs  the torch decode alone                     14 x 480 x 640 payloads
  C  dsec_flow_png16(flow)                        vs  a torch mirror of scale_optical_flow (torch.where for the boolean
     assignment, which would synchronise) + the quantisation                                     1 and 14 x 480 x 640 flows

The yardstick is the chain, never the new code against itself: `fused_not_slower` is median(fused) <= median(chain) + spread, the
spread being the larger interquartile range of the two.  For A the k_ingest_* kernels are also timed one by one (ops.KernelTimer)
with and without the map: what gathering in each of the kernels costs against writing the rectified floats once.
Writes profiles/dsec_io.json (tagged with build.source_hash()):
    python tools/dsec_io_probe.py [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import LossFactory, build, ops  # noqa: E402
from motionpriorcmax_amd.utils import (calculate_flow_error, dsec_flow_error, dsec_flow_png16, dsec_flow_targets,  # noqa: E402
                                       ingest_events)

CALLS, WARM, COPIES = 30, 5, 10
H, W, NB = 480, 640, 15
POOL_BYTES = 300e6
dev = torch.device('cuda:0')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3          # us


def stats(v):
    q = statistics.quantiles(v, n=4)
    return {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2), 'iqr': round(q[2] - q[0], 2)}


class Pool:
    """n buffers made by make(i), handed out round robin."""

    def __init__(self, make, bytes_each):
        self.items = [make(i) for i in range(max(2, int(POOL_BYTES // bytes_each) + 1))]
        self.k = 0

    def next(self):
        self.k += 1
        return self.items[self.k % len(self.items)]


def compare(fused, chain, nbytes, kernels_of=None):
    """fused / chain: callables; nbytes: what the fused call reads and writes once."""
    src = Pool(lambda i: torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 255), nbytes // 2)
    dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)

    def cpy():
        for _ in range(COPIES):
            dst.copy_(src.next())
    for _ in range(WARM):
        fused(); chain(); cpy()
    tf, tc, tk = [], [], []
    for _ in range(CALLS):
        tf.append(timed(fused)); tc.append(timed(chain)); tk.append(timed(cpy) / COPIES)
    sf, sc = stats(tf), stats(tc)
    spread = max(sf['iqr'], sc['iqr'])
    r = {'fused_us': sf, 'chain_us': sc, 'copy_same_bytes_us': stats(tk), 'bytes': nbytes, 'spread_us': spread,
         'chain_over_fused': round(sc['median'] / sf['median'], 2), 'fused_not_slower': bool(sf['median'] <= sc['median'] + spread)}
    if kernels_of:
        for name, fn in kernels_of.items():
            with ops.KernelTimer() as kt:
                for _ in range(12):
                    fn()
            r['kernels_' + name] = {n: {'launches_per_call': v['launches'] / 12, 'avg_us': round(v['avg_us'], 2)} for n, v in kt.summary().items()}
    del src, dst
    torch.cuda.empty_cache()
    return r


def probe_ingest(res):
    B, N = 14, 200000
    g = torch.Generator(device=dev).manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing='ij')
    m = torch.stack((xx + 3 * torch.sin(yy / 70), yy + 3 * torch.cos(xx / 90)), -1).contiguous()
    counts = torch.full((B,), N, dtype=torch.int32)

    def make(i):
        x = torch.randint(0, W, (B, N), generator=g, device=dev, dtype=torch.int32)
        y = torch.randint(0, H, (B, N), generator=g, device=dev, dtype=torch.int32)
        t = torch.sort(torch.randint(0, 100000, (B, N), generator=g, device=dev), dim=1).values + 51_000_000_000
        p = (torch.rand(B, N, generator=g, device=dev) > 0.45).float()
        return x, y, t, p
    pool = Pool(make, B * N * 20)
    cfg = dict(image_shape=(H, W), num_tref=1, num_bins=NB, num_knn=32, smooth_weight=0.003, lut_superpixel_size=4,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    loss = LossFactory.get_loss_calculator('FOCUS', cfg)
    for tag, order in (('plain', None), ('bucket_order', loss)):
        def fused():
            x, y, t, p = pool.next()
            return ingest_events(x, y, t, p, counts, (H, W), NB, want_voxel_input=True, order_for=order, rectify_map=m)

        def chain():
            x, y, t, p = pool.next()
            r = m[y.long(), x.long()]
            return ingest_events(r[..., 0].contiguous(), r[..., 1].contiguous(), t, p, counts, (H, W), NB, want_voxel_input=True, order_for=order)
        a, b = fused(), chain()          # (different buffers: shapes only)
        x, y, t, p = pool.items[0]
        r = m[y.long(), x.long()]
        a = ingest_events(x, y, t, p, counts, (H, W), NB, want_voxel_input=True, rectify_map=m)
        b = ingest_events(r[..., 0].contiguous(), r[..., 1].contiguous(), t, p, counts, (H, W), NB, want_voxel_input=True)
        same = bool(torch.equal(a['events'], b['events']) and torch.equal(a['xytp'], b['xytp']))
        nbytes = B * N * 20 + H * W * 8 + int(a['events'].numel()) * 4 + B * N * 16
        res['A_ingest_' + tag] = dict(compare(fused, chain, nbytes, {'with_map': fused, 'float_path_after_gather': chain}),
                                      workload=dict(B=B, N=N, map=[H, W], voxel_rows=True), equal_to_chain=same)
        print('A', tag, json.dumps(res['A_ingest_' + tag]), flush=True)
    del pool
    torch.cuda.empty_cache()


def torch_decode(png):
    """loader.py:174-180 with torch on the device (uint16 through its bit pattern: torch has few uint16 kernels)."""
    f = (png.view(torch.int16).to(torch.int32) & 0xFFFF).float()
    flow = torch.stack(((f[..., 1] - 2**15) / 128., (f[..., 0] - 2**15) / 128.), dim=1)
    return flow, f[..., 2] != 0


def probe_payload(res):
    B = 14
    g = torch.Generator(device=dev).manual_seed(2)

    def make(i):
        png = torch.randint(0, 65536, (B, H, W, 3), generator=g, device=dev, dtype=torch.int32).to(torch.int16).view(torch.uint16)
        pred = torch.randn(B, 2, H, W, generator=g, device=dev) * 90
        return png, pred
    pool = Pool(make, B * H * W * 14)
    png, pred = pool.items[0]
    a, (fl, va) = dsec_flow_error(png, pred), torch_decode(png)
    b = calculate_flow_error(fl, pred, va)
    t = dsec_flow_targets(png)

    def chain():
        png_, pred_ = pool.next()
        flow_, valid_ = torch_decode(png_)
        return calculate_flow_error(flow_, pred_, valid_)
    res['B_error'] = dict(compare(lambda: dsec_flow_error(*pool.next()), chain, B * H * W * 14,
                                  {'fused': lambda: dsec_flow_error(*pool.next()), 'chain': chain}),
                          workload=dict(B=B, H=H, W=W), equal_to_chain=bool(all(torch.equal(a[k], b[k]) for k in a)))
    print('B error', json.dumps(res['B_error']), flush=True)
    res['B_targets'] = dict(compare(lambda: dsec_flow_targets(pool.next()[0]), lambda: torch_decode(pool.next()[0]), B * H * W * 15,
                                    {'fused': lambda: dsec_flow_targets(pool.next()[0])}),
                            workload=dict(B=B, H=H, W=W), equal_to_chain=bool(torch.equal(t['forward_flow'], fl) and torch.equal(t['flow_valid'], va)))
    print('B targets', json.dumps(res['B_targets']), flush=True)
    del pool
    torch.cuda.empty_cache()


def torch_export(flow, max_magnitude=60.0):
    """scripts/dsec_inference.py:33-49 with torch on the device."""
    u, v = flow[:, 0], flow[:, 1]
    mag = torch.sqrt(u**2 + v**2)
    ex = mag > max_magnitude
    u = torch.where(ex, (u / mag) * max_magnitude, u)
    v = torch.where(ex, (v / mag) * max_magnitude, v)
    q = lambda c: (c * 128 + 2**15).to(torch.int32).to(torch.int16)
    return torch.stack((q(v), q(u), torch.zeros_like(u, dtype=torch.int16)), dim=-1).view(torch.uint16)


def probe_export(res):
    g = torch.Generator(device=dev).manual_seed(3)
    for B in (1, 14):
        pool = Pool(lambda i: torch.randn(B, 2, H, W, generator=g, device=dev) * 40, B * H * W * 8)
        f = pool.items[0]
        same = bool(torch.equal(dsec_flow_png16(f).view(torch.int16), torch_export(f).view(torch.int16)))
        res[f'C_export_B{B}'] = dict(compare(lambda: dsec_flow_png16(pool.next()), lambda: torch_export(pool.next()), B * H * W * 14,
                                             {'fused': lambda: dsec_flow_png16(pool.next())}),
                                     workload=dict(B=B, H=H, W=W, pool_buffers=len(pool.items)), equal_to_chain=same)
        print('C', B, json.dumps(res[f'C_export_B{B}']), flush=True)
        del pool
        torch.cuda.empty_cache()


def main(out):
    if not torch.cuda.is_available():
        raise SystemExit('this probe measures on the GPU; there is none here')
    res = {'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(dev), 'calls': CALLS, 'warmup': WARM,
           'timing': 'HIP events around one call (host launch work included; ingest reads two integers back, in both forms); fused, '
                     'chain and copy alternate call by call; every call works on another buffer of a pool larger than the Infinity '
                     'Cache.  spread_us = the larger interquartile range of fused and chain.'}
    probe_ingest(res)
    probe_payload(res)
    probe_export(res)
    res['fused_not_slower_everywhere'] = all(v['fused_not_slower'] for v in res.values() if isinstance(v, dict) and 'fused_not_slower' in v)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'dsec_io.json'))
