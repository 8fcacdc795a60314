#!/usr/bin/env python3
"""The RAFT-spline validation metrics as one fused reduction (utils.trajectory_val_metrics, csrc/val_metrics.hip) against what the
package offered before for the same 45 scalars: utils.flows_from_bezier (its kernel: the [M, B, 2, H, W] predictions are written)
plus a plain-torch mirror of the reference's metric chain on the device (src/modules/utils.py:85-296 operator for operator: the two
[N, 3, H, W] concatenations of ae_masked, the boolean gathers, the `if denominator == 0` host synchronisations), on the same GPU in
ONE process, A and B alternating: median of 7 blocks of 10 steps after warm-up, host clock ending in a device synchronise.
EVIMO2 size: B = 6, 384 x 512, d = 10, M = 6, C = 65, with flow_valid.
Per-kernel times of the fused call from ops.KernelTimer, and the bandwidth they amount to over the bytes the algorithm needs
(computed from the shapes: ev_repr 4C, ground truth 8M, validity M, logits 36 bytes per pixel).  The two paths' results are compared
at this size before anything is timed.  Writes profiles/val_metrics.json (tagged with build.source_hash()):
    python tools/val_metrics_probe.py [out.json]"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import ops, utils, build  # noqa: E402

BLOCKS, STEPS, WARM = 7, 10, 3
B, H, W, D, M, C = 6, 384, 512, 10, 6, 65
TIMES = [0.15, 0.3, 0.5, 0.65, 0.85, 1.0]
dev = torch.device('cuda:0')


# ---- the reference's chain in plain torch (utils.py:85-296), as a user of the parent commit would run it on the device
def _epe(p, g, k=None):
    e = (p - g).square().sum(1).sqrt()
    if k is None:
        return e.mean()
    n = k.sum()
    if n == 0:                                   # (a host synchronisation, as in the reference)
        return None
    return e[k].sum() / n


def _ae(p, g, k=None):
    one = torch.ones_like(p[:, :1])
    pe, ge = torch.cat((p, one), 1), torch.cat((g, one), 1)
    c = (pe * ge).sum(1) / (torch.linalg.norm(pe, dim=1) * torch.linalg.norm(ge, dim=1))
    c[c > 1.0] = 1.0
    c[c < -1.0] = -1.0
    a = torch.acos(c) / math.pi * 180
    return a.mean() if k is None else a[k].sum() / k.sum()


def _npe(p, g, k, npx):
    gm, em = torch.linalg.norm(g, dim=1), torch.linalg.norm(p - g, dim=1)
    if k is not None:
        n = k.sum()
        assert n > 0                             # (a host synchronisation, as in the reference)
        rel = torch.zeros_like(em)
        rel[k] = em[k] / gm[k].clip(min=1e-6)
    else:
        rel = em / gm.clip(min=1e-6)
    hit = (em > npx) & (rel >= 0.05)
    return (hit[k].sum() / n if k is not None else hit.float().mean()) * 100


def _flow_error(g, p, k=None):
    fm = ~torch.isinf(g[:, [0]]) & ~torch.isinf(g[:, [1]]) & (g[:, [0]].abs() > 0) & (g[:, [1]].abs() > 0)
    tm = fm if k is None else (k & fm)
    gm, pm = g * tm, p * tm
    n = tm.sum(dim=(1, 2, 3)) + 1e-5
    e = torch.linalg.norm(gm - pm, dim=1)
    out = {'EPE': (e.sum(dim=(1, 2)) / n).mean()}
    for j in (1, 2, 3):
        out[f'{j}PE'] = ((e > j).sum(dim=(1, 2)) / n).mean()
    u, v, ug, vg = pm[:, 0], pm[:, 1], gm[:, 0], gm[:, 1]
    c = ((1.0 + u * ug + v * vg) / (torch.sqrt(1 + u * u + v * v) * torch.sqrt(1 + ug * ug + vg * vg))).clamp(-1, 1)
    out['AE'] = (torch.acos(c).sum(dim=(1, 2)) / n).mean() * (180.0 / math.pi)
    return out


def _multi(prefix, preds, gts, masks, out):
    ks = masks if masks is not None else [None] * len(preds)
    epes = [x for x in (_epe(p, g, k) for p, g, k in zip(preds, gts, ks)) if x is not None]
    if epes:
        out[prefix + 'epe_multi'] = sum(epes) / len(epes)
    out[prefix + 'ae_multi'] = sum(_ae(p, g, k) for p, g, k in zip(preds, gts, ks)) / len(preds)
    src, tgt = torch.stack(preds), torch.stack(gts)
    vm = torch.stack(masks) if masks is not None else None
    h, w = src.shape[-2:]
    err = _flow_error(tgt.reshape(-1, 2, h, w), src.reshape(-1, 2, h, w), None if vm is None else vm.reshape(-1, h, w)[:, None])
    out[prefix + 'T3PE'], out[prefix + 'TEPE'], out[prefix + 'TAE'] = err['3PE'], err['EPE'], err['AE']
    for i in range(len(preds)):
        out[f'{prefix}EPE_STEP{str(i).zfill(2)}'] = _flow_error(tgt[i], src[i], None if vm is None else vm[i][:, None])['EPE']


def parent_path(p, m, gt, valid, ev):
    flows = utils.flows_from_bezier(p, TIMES, up_mask=m)                  # the parent's kernel: [M, B, 2, H, W] written
    preds, gts = list(flows.unbind(0)), list(gt.unbind(1))
    out = {}
    event_mask = ev.abs().any(dim=1) > 0
    for prefix, k in (('val/', None), ('val/masked_', event_mask)):
        out[prefix + 'epe'] = _epe(preds[-1], gts[-1], k)
        out[prefix + 'ae'] = _ae(preds[-1], gts[-1], k)
        for j in (1, 2, 3):
            out[f'{prefix}{j}pe'] = _npe(preds[-1], gts[-1], k, j)
    _multi('val/', preds, gts, None, out)
    _multi('val/ev_masked_', preds, gts, [event_mask & valid[:, s] for s in range(M)], out)
    _multi('val/masked_', preds, gts, [valid[:, s] for s in range(M)], out)
    lin = [t * preds[-1] for t in TIMES]
    out['val/epe_multi_lin'] = sum(_epe(a, g) for a, g in zip(lin, gts)) / M
    out['val/ae_multi_lin'] = sum(_ae(a, g) for a, g in zip(lin, gts)) / M
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def main(out_path):
    g = torch.Generator().manual_seed(15)
    h, w = H // 8, W // 8
    p = (torch.randn(B, 2 * D, h, w, generator=g) * 0.5).to(dev)
    m = (torch.randn(B, 576, h, w, generator=g) * 2.0).to(dev)
    ts = torch.tensor(TIMES, dtype=torch.float32, device=dev)
    gt = utils.flows_from_bezier(p, TIMES, up_mask=m).permute(1, 0, 2, 3, 4).contiguous()
    gt = gt + torch.randn(gt.shape, generator=g).to(dev) * 1.5
    gt[(torch.rand(B, M, 1, H, W, generator=g) < 0.05).to(dev).expand_as(gt)] = 0.0
    valid = (torch.rand(B, M, H, W, generator=g) < 0.7).to(dev)
    ev = (torch.randn(B, C, H, W, generator=g) * (torch.rand(B, C, H, W, generator=g) < 0.02)).to(dev)

    def fused():
        return utils.trajectory_val_metrics(gt, ts, params=p, up_mask=m, flow_valid=valid, ev_repr=ev)

    def parent():
        return parent_path(p, m, gt, valid, ev)

    a, b = fused()[0], parent()
    worst = max((abs(a[k].item() - b[k].item()) / max(abs(b[k].item()), 1e-30), k) for k in b)
    assert sorted(a) == sorted(b) and len(a) == 45, (len(a), len(b))
    print('largest relative difference between the two paths:', worst, flush=True)
    modes = {'parent_flows_plus_torch_chain': parent, 'fused': fused, 'parent_flows_kernel_only': lambda: utils.flows_from_bezier(p, TIMES, up_mask=m)}
    for fn in modes.values():
        for _ in range(WARM):
            fn()
    samples = {k: [] for k in modes}
    for _ in range(BLOCKS):
        for k, fn in modes.items():
            samples[k].append(timed(fn))
    res = {'source_hash': build.source_hash(), 'method': f'one process, A/B alternating, median of {BLOCKS} blocks x {STEPS} steps after '
           f'{WARM} warm-up steps; host clock ending in torch.cuda.synchronize(); per-kernel: ops.KernelTimer',
           'shape': dict(B=B, image=[H, W], d=D, M=M, C=C, flow_valid=True),
           'largest_relative_difference_between_the_paths': {'value': worst[0], 'key': worst[1]}}
    for k, v in samples.items():
        res[k] = {'median_ms': round(statistics.median(v), 4), 'blocks_ms': [round(x, 4) for x in v]}
    with ops.KernelTimer() as kt:
        for _ in range(5):
            fused()
    kern = {k: {'launches_per_call': v['launches'] / 5, 'avg_us': round(v['avg_us'], 2)}
            for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]['total_us'])}
    kernel_us = sum(v['avg_us'] * v['launches_per_call'] for v in kern.values())
    per_px = dict(ev_repr=4 * C, ground_truth=8 * M, validity=M, logits=36)
    total = sum(per_px.values()) * B * H * W
    res['kernels'] = kern
    res['fused_kernels_us'] = round(kernel_us, 2)
    res['bytes'] = dict(per_pixel=per_px, per_pixel_total=sum(per_px.values()), total=total)
    res['achieved_GBps_over_the_kernels'] = round(total / kernel_us / 1e3, 1)
    res['achieved_GBps_of_k_val_evmask_over_ev_repr'] = round(4 * C * B * H * W / kern['k_val_evmask']['avg_us'] / 1e3, 1)
    res['parent_over_fused'] = round(res['parent_flows_plus_torch_chain']['median_ms'] / res['fused']['median_ms'], 2)
    res['fused_faster_than_parent'] = bool(res['fused']['median_ms'] < res['parent_flows_plus_torch_chain']['median_ms'])
    print(json.dumps({k: res[k]['median_ms'] for k in modes}), json.dumps(kern), res['achieved_GBps_over_the_kernels'], res['parent_over_fused'], flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', out_path)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'val_metrics.json'))
