#!/usr/bin/env python3
"""utils.flow_targets(dataset='evimo2') (csrc/flow_targets.hip, one launch) against a plain-torch mirror of the operator chain the
reference's loader runs (two isnan, an and, a masked assignment, three F.interpolate, two strided in-place multiplies;
src/loader/evimo2/datasubset.py:171-188), both on the same GPU tensors in ONE process, alternating call by call: HIP events around every
call, median of CALLS calls after warm-up.  The shipped shape: S = 6 steps, 480 x 640 -> 384 x 512, at B = 6 and B = 1, ~20 % NaN,
an fp32 object-id mask.  Every call reads another buffer of a pool larger than the 256 MB Infinity Cache, so that the input comes
from HBM as a fresh batch does; the same holds for the plain device-to-device copy that moves the same number of bytes (half read,
half written), which is the streaming rate the kernel is compared with.
Algorithmic bytes: the raw flow and the id mask read once; flow, validity bytes and id mask written once.  Per-kernel time from
ops.KernelTimer.  Writes profiles/flow_targets.json (tagged with build.source_hash()):
    python tools/flow_targets_probe.py [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from motionpriorcmax_amd import build, ops  # noqa: E402
from motionpriorcmax_amd.utils import flow_targets  # noqa: E402

CALLS, WARM, COPIES = 30, 5, 10
S, H, W, HO, WO = 6, 480, 640, 384, 512
POOL_BYTES = 600e6
PEAK_TBPS = 8.0
dev = torch.device('cuda:0')


def synth(B, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randn(B, S, 2, H, W, generator=g, device=dev) * 5.0
    blob = F.interpolate((torch.rand(B, S, H // 16, W // 16, generator=g, device=dev) < 0.15).float(), size=(H, W), mode='nearest') > 0
    raw[blob[:, :, None].expand_as(raw)] = float('nan')
    raw[torch.rand(B, S, 2, H, W, generator=g, device=dev) < 0.03] = float('nan')
    ids = torch.randint(0, 256, (B, H, W), generator=g, device=dev).float()
    return raw, ids


def mirror(raw, ids):
    """The loader's chain, batched over (B, S).  It zeroes the NaN of `raw` in place, as the loader does with the array it owns:
    the caller hands it a fresh clone, made outside the timed window (which leaves that clone warm in the caches: in the
    mirror's favour)."""
    B = raw.shape[0]
    valid = (~torch.isnan(raw[:, :, 0])) & (~torch.isnan(raw[:, :, 1]))
    flow = raw
    flow[torch.isnan(flow)] = 0.
    flow = F.interpolate(flow.flatten(0, 1), size=[HO, WO], mode='bilinear', align_corners=False).unflatten(0, (B, S))
    valid = F.interpolate(valid.float(), size=[HO, WO], mode='nearest').bool()
    idm = F.interpolate(ids[:, None], size=[HO, WO], mode='nearest')[:, 0]
    flow[:, :, 0] *= WO / W
    flow[:, :, 1] *= HO / H
    return flow, valid, idm


def timed(fn, setup=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    arg = setup() if setup else None
    torch.cuda.synchronize(dev)
    e0.record()
    fn(arg) if setup else fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3          # us


def stats(v):
    return {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}


def main(out):
    if not torch.cuda.is_available():
        raise SystemExit('this probe measures on the GPU; there is none here')
    res = {'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(dev), 'calls': CALLS, 'warmup': WARM,
           'shape': dict(S=S, H=H, W=W, Ho=HO, Wo=WO), 'peak_TBps': PEAK_TBPS,
           'timing': 'HIP events around one call (host launch work included); library, mirror and copy alternate call by call; every '
                     'call reads another buffer of a pool larger than the Infinity Cache', 'batches': {}}
    for B in (6, 1):
        raw0, ids0 = synth(B, seed=30 + B)
        n_pool = max(2, int(POOL_BYTES // (raw0.numel() * 4)) + 1)
        pool = [(raw0, ids0)] + [(raw0.clone(), ids0.clone()) for _ in range(n_pool - 1)]
        need = raw0.numel() * 4 + ids0.numel() * 4 + B * S * HO * WO * (2 * 4 + 1) + B * HO * WO * 4
        src = [torch.empty(need // 2, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(max(2, int(POOL_BYTES // (need // 2)) + 1))]
        dst = torch.empty(need // 2, dtype=torch.uint8, device=dev)
        a, (m_flow, m_valid, m_id) = flow_targets(raw0, (HO, WO), dataset='evimo2', id_mask=ids0), mirror(raw0.clone(), ids0)
        max_diff = float((a['flow'] - m_flow).abs().max())
        masks_equal = bool(torch.equal(a['flow_valid'], m_valid) and torch.equal(a['id_mask'], m_id))
        k = [0]

        def nxt(p):
            k[0] += 1
            return p[k[0] % len(p)]

        def lib():
            raw, ids = nxt(pool)
            return flow_targets(raw, (HO, WO), dataset='evimo2', id_mask=ids)

        def mir_setup():
            raw, ids = nxt(pool)
            return raw.clone(), ids

        def mir(arg):
            return mirror(*arg)

        def cpy():                                # COPIES back to back: the launch latency of one copy would rival a B = 1 copy itself
            for _ in range(COPIES):
                dst.copy_(nxt(src))
        for _ in range(WARM):
            lib(); mir(mir_setup()); cpy()
        t_lib, t_mir, t_cpy = [], [], []
        for _ in range(CALLS):
            t_lib.append(timed(lib)); t_mir.append(timed(mir, mir_setup)); t_cpy.append(timed(cpy) / COPIES)
        with ops.KernelTimer() as kt:
            for _ in range(n_pool + 5):
                lib()
        kern = {n: {'launches_per_call': v['launches'] / (n_pool + 5), 'avg_us': round(v['avg_us'], 2)} for n, v in kt.summary().items()}
        kernel_us = sum(v['avg_us'] * v['launches_per_call'] for v in kern.values())
        ml, mm, mc = statistics.median(t_lib), statistics.median(t_mir), statistics.median(t_cpy)
        r = {'workload': dict(B=B, S=S, nan_share=round(float(torch.isnan(raw0).float().mean()), 3), pool_buffers=n_pool),
             'library_us': stats(t_lib), 'mirror_us': stats(t_mir), 'copy_us': stats(t_cpy),
             'mirror_over_library': round(mm / ml, 2), 'library_not_slower': bool(ml <= mm),
             'max_abs_flow_difference_to_mirror': max_diff, 'masks_equal_mirror': masks_equal,
             'kernels': kern, 'kernel_us_per_call': round(kernel_us, 2), 'algorithmic_bytes': need,
             'kernel_TBps': round(need / kernel_us / 1e6, 3) if kernel_us else None,
             'kernel_fraction_of_peak': round(need / kernel_us / 1e6 / PEAK_TBPS, 3) if kernel_us else None,
             'call_TBps': round(need / ml / 1e6, 3), 'copy_TBps_same_bytes': round(need / mc / 1e6, 3),
             'kernel_over_copy_rate': round((need / kernel_us) / (need / mc), 3) if kernel_us else None}
        res['batches'][f'B{B}'] = r
        print(f'B={B}', json.dumps(r), flush=True)
        del pool, src, dst
        torch.cuda.empty_cache()
    res['library_not_slower_at_both_shapes'] = all(r['library_not_slower'] for r in res['batches'].values())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'flow_targets.json'))
