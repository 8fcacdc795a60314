"""An own restatement of the RAFT-spline validation metrics (reference src/modules/raft_spline.py:159-194 over src/modules/utils.py
:67-74, 85-296, 335-541), written from the formulas and run in float64: test code only, the package never imports it.

    curve_flows(params, mask, times, scale)          the convex-upsampled Bezier curves at `times`, [M, B, 2, 8h, 8w]
    event_mask(ev_repr)                              E = any channel != 0 (a NaN counts)
    metrics(pred, gt, ts, flow_valid, E)             -> (values, updated): dicts over the logged names, Python floats / ints
    push_off_thresholds(pred, gt)                    moves ground-truth vectors until every count metric is exact in fp32 (below)
    combine(list of (values, updated))               the Metric rule over batches: sum of the updated values / their number

Everything runs in the dtype of `pred` / `gt` (torch, CPU): float64 is the oracle; the same code in fp32 does the reference's
operations at the reference's precision, and the distance between the two is the stand-in for the reference's own rounding noise
where no fixture recorded it (tests/test_gpu_val_metrics.py: the random seeds)."""
import math

import numpy as np
import torch

SINGLE = ('epe', 'ae', '1pe', '2pe', '3pe')


def curve_flows(params, mask, times, scale=1.0):
    P, Mk = params, mask
    B, c2, h, w = P.shape
    d, H, W = c2 // 2, 8 * h, 8 * w
    y, x = torch.arange(H), torch.arange(W)
    cy, sy, cx, sx = (y // 8)[:, None], (y % 8)[:, None], (x // 8)[None, :], (x % 8)[None, :]
    wk = torch.softmax(Mk.view(B, 9, 8, 8, h, w)[:, :, sy, sx, cy, cx], dim=1)                  # [B, 9, H, W]
    P0 = torch.nn.functional.pad(P, (1, 1, 1, 1))
    up = sum(wk[:, None, k] * 8 * P0[:, :, cy + k // 3, cx + k % 3] for k in range(9))          # [B, 2d, H, W]
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    bm = np.stack([math.comb(d, i) * (1 - t) ** (d - i) * t ** i for i in range(1, d + 1)], axis=1)
    bm = torch.from_numpy(bm).float().to(P.dtype)                  # float64 on the host, then fp32: bezier.py:102-107
    return torch.einsum('bcjhw,tj->tbchw', up.view(B, 2, d, H, W), bm) * scale


def event_mask(ev_repr):
    return (ev_repr != 0).any(dim=1)


def _per_pixel(P, G):
    """e, a (degrees), r_1..3 of predictions P and ground truth G, both [B, 2, H, W]."""
    e = ((P - G) ** 2).sum(1).sqrt()
    num = (P * G).sum(1) + 1
    den = ((P ** 2).sum(1) + 1).sqrt() * ((G ** 2).sum(1) + 1).sqrt()
    a = torch.acos((num / den).clamp(-1, 1)) / math.pi * 180
    rel = e / (G ** 2).sum(1).sqrt().clamp(min=1e-6)
    return e, a, [(e > k) & (rel >= 0.05) for k in (1, 2, 3)]


def _batch(e, a, K):
    """(epe or None, ae) over the mask K (None: every pixel), normalised over the whole batch."""
    if K is None:
        return float(e.mean()), float(a.mean())
    n = int(K.sum())
    return (float(e[K].sum()) / n if n else None), (float(a[K].sum()) / n if n else float('nan'))


def _multi(es, As, Ks, gts, prefix, values, updated):
    """The eleven `multi` keys of one mask set; Ks: a mask per step or None."""
    M, B = len(es), es[0].shape[0]
    steps = [_batch(es[m], As[m], None if Ks is None else Ks[m]) for m in range(M)]
    epes = [s[0] for s in steps if s[0] is not None]
    values[prefix + 'epe_multi'] = sum(epes) / len(epes) if epes else float('nan')
    updated[prefix + 'epe_multi'] = 1 if epes else 0
    values[prefix + 'ae_multi'] = sum(s[1] for s in steps) / M
    tepe = t3pe = tae = 0.0
    for m in range(M):
        F = (gts[m][:, 0] != 0) & (gts[m][:, 1] != 0) & ~torch.isinf(gts[m][:, 0]) & ~torch.isinf(gts[m][:, 1])
        if Ks is not None:
            F = F & Ks[m]
        step = 0.0
        for n in range(B):                                             # per IMAGE: sum over its mask / (its count + 1e-5)
            cnt = int(F[n].sum()) + 1e-5
            step += float(es[m][n][F[n]].sum()) / cnt
            t3pe += int((es[m][n][F[n]] > 3).sum()) / cnt
            tae += float(As[m][n][F[n]].sum()) / cnt
        tepe += step
        values[f'{prefix}EPE_STEP{str(m).zfill(2)}'] = step / B
    values[prefix + 'TEPE'], values[prefix + 'T3PE'], values[prefix + 'TAE'] = tepe / (M * B), t3pe / (M * B), tae / (M * B)
    for k in ['ae_multi', 'TEPE', 'T3PE', 'TAE'] + [f'EPE_STEP{str(m).zfill(2)}' for m in range(M)]:
        updated[prefix + k] = 1


def metrics(pred, gt, ts, flow_valid, E):
    """pred [M, B, 2, H, W], gt [B, M, 2, H, W], ts [M], flow_valid [B, M, H, W] bool or None, E [B, H, W] bool."""
    M = pred.shape[0]
    values, updated = {}, {}
    gts = [gt[:, m] for m in range(M)]
    pp = [_per_pixel(pred[m], gts[m]) for m in range(M)]
    es, As = [p[0] for p in pp], [p[1] for p in pp]
    for prefix, K in (('val/', None), ('val/masked_', E)):
        n = es[-1].numel() if K is None else int(K.sum())
        epe, ae = _batch(es[-1], As[-1], K)
        row = [epe, ae] + [100.0 * int((r if K is None else r[K]).sum()) / n if n else None for r in pp[-1][2]]
        for k, v in zip(SINGLE, row):
            # an empty mask: EPE skips, NPE raises in the reference (utils.py:199) -- the whole row counts as not updated
            values[prefix + k], updated[prefix + k] = (v, 1) if n else (float('nan'), 0)
    _multi(es, As, None, gts, 'val/', values, updated)
    _multi(es, As, [E & flow_valid[:, m] for m in range(M)] if flow_valid is not None else [E] * M, gts, 'val/ev_masked_', values, updated)
    _multi(es, As, [flow_valid[:, m] for m in range(M)] if flow_valid is not None else None, gts, 'val/masked_', values, updated)
    lin = [_per_pixel(float(np.float32(ts[m])) * pred[-1], gts[m]) for m in range(M)]              # utils.py:67-74
    values['val/epe_multi_lin'] = sum(float(p[0].mean()) for p in lin) / M
    values['val/ae_multi_lin'] = sum(float(p[1].mean()) for p in lin) / M
    updated['val/epe_multi_lin'] = updated['val/ae_multi_lin'] = 1
    return values, updated


def threshold_violations(pred, gt):
    """[B, M, H, W] bool: pixels where a count metric could flip under fp32 rounding -- |e - k| < 1e-4 for k = 1, 2, 3, |e / |G| - 0.05| <
    1e-5, or a ground-truth component in (0, 1e-6).  float64 inputs."""
    P = pred.permute(1, 0, 2, 3, 4)
    e = ((P - gt) ** 2).sum(2).sqrt()
    g = (gt ** 2).sum(2).sqrt()
    bad = torch.zeros_like(e, dtype=torch.bool)
    for k in (1, 2, 3):
        bad |= (e - k).abs() < 1e-4
    bad |= (e / g.clamp(min=1e-6) - 0.05).abs() < 1e-5
    bad |= ((gt.abs() > 0) & (gt.abs() < 1e-6)).any(2)
    return bad


def push_off_thresholds(pred, gt):
    """gt (fp32, modified in place) with every violating vector moved in x by 1/256 per round until none is left."""
    for _ in range(32):
        bad = threshold_violations(pred.double(), gt.double())
        if not bad.any():
            return gt
        gt[:, :, 0][bad] += 1.0 / 256
    raise AssertionError('could not clear the thresholds')


def combine(batches):
    """Metric.compute over per-batch (values, updated): sum of the values whose flag is set / their number."""
    out = {}
    for k in batches[0][0]:
        vals = [v[k] for v, u in batches if u[k]]
        out[k] = sum(vals) / len(vals) if vals else float('nan')
    return out


def bound(x64, err):
    """The project's rule (tests/test_cvx_traj_host.py): max(4 * the reference's own fp32 error, fp32 output rounding)."""
    return max(4.0 * err, 2.0 ** -22 * abs(x64))
