#!/usr/bin/env python3
"""Fixtures g15_val_<case>.npz for the RAFT-spline validation metrics (utils.trajectory_val_metrics, utils.TrajectoryValMetrics):
what the UNMODIFIED reference logs in `RAFTSplineModule.validation_step` (src/modules/raft_spline.py:159-194) for one batch,
computed by the unmodified functions of src/modules/utils.py (epe_masked, epe_masked_multi, ae_masked, ae_masked_multi,
n_pixel_error_masked, calculate_flow_error, calculate_trajectory_flow_error, predictions_from_lin_assumption) in fp32, for six
steps also through its Metric classes (asserted equal), beside the same chain in float64 and the distance between the two -- the
tests derive their tolerances from it.

    python tools/gen_golden_val.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_cvx.py: oracle/stubs stands in for the third-party packages the reference imports, tools/stubs for torchmetrics
(a Metric with add_state, nothing else), the reference's own files are imported as they are, and only DATA is written.
Deterministic (seeded, one thread): a second run reproduces the files bit for bit.

Every file holds
  times [M], scale, flow_gt [B, M, 2, H, W], ev_repr [B, C, H, W], flow_valid [B, M, H, W] (absent: the batch has none)
  params [B, 2d, h, w], mask [B, 576, h, w]      (curve cases)
  pred [M, B, 2, H, W]                           the reference's fp32 predictions: create_upsampled(mask).get_flow_from_reference(t)
                                                 per step (a drawn tensor in the `flows` case d); case c keeps it in
                                                 g15_val_c_pred.npz (it does not compress: 0.7 MB)
  keys, ref (fp32), updated, f64, err            per logged name: the reference's value, whether its Metric.update adds it, the
                                                 float64 value, |ref - f64| (0 where both are NaN)
An empty mask makes the reference's NPE raise (utils.py:199); the five singles of that mask are then written as NaN / updated 0
(case e): that row is unpinned.

Threshold margin: the count metrics compare e with 1, 2, 3 and e / |G| with 0.05.  The generator asserts, in float64 and for
every pixel and step, |e - k| >= 1e-4, |e / |G| - 0.05| >= 1e-5 and no ground-truth component in (0, 1e-6), moving offending
ground-truth vectors by 1/256 until it holds (deterministically): fp32 rounding then cannot flip a count, and the count metrics
are exact.  The ground truth lies on a grid of 1/64 (1/8 in case c) and the logits on a grid of 1/2 so that the files stay small."""
import argparse
import os
import sys

import numpy as np

from gen_golden_cvx import save_npz

T6 = [0.15, 0.3, 0.5, 0.65, 0.85, 1.0]
CASES = [  # name, B, d (0: `flows` mode), (h, w) or (H, W), times, C, flow_valid, scale, ground-truth grid
    ('a', 2, 10, (2, 3), T6, 5, True, 1.0, 64),
    ('b', 1, 3, (3, 5), T6, 1, False, 2.0, 64),
    ('c', 3, 10, (3, 33), T6, 3, True, 1.0, 8),
    ('d', 2, 0, (13, 21), [0.25, 0.6, 1.0], 2, True, 1.0, 64),
    ('e', 1, 4, (2, 2), T6, 2, True, 1.0, 64),
]
SINGLE = ('epe', 'ae', '1pe', '2pe', '3pe')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'oracle', 'stubs'))
    sys.path.insert(1, os.path.join(root, 'tools', 'stubs'))
    sys.path.insert(2, args.ref)
    import torch
    from src.models.raft_spline.curves import BezierCurves          # reference, unmodified
    from src.modules import utils as R                              # reference, unmodified

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)

    def violations(pred64, gt64):
        """[B, M, H, W]: the pixels inside a threshold margin (float64)."""
        P = pred64.permute(1, 0, 2, 3, 4)
        e = (P - gt64).square().sum(2).sqrt()
        g = gt64.square().sum(2).sqrt()
        bad = ((gt64.abs() > 0) & (gt64.abs() < 1e-6)).any(2) | ((e / g.clamp(min=1e-6) - 0.05).abs() < 1e-5)
        for k in (1, 2, 3):
            bad |= (e - k).abs() < 1e-4
        return bad

    def npe64(pred, gt, mask, k):
        """n_pixel_error_masked (utils.py:186-218) with a float64 quotient: the reference divides the count in fp32 whatever the inputs."""
        e = (pred - gt).square().sum(1).sqrt()
        hit = (e > k) & (e / gt.square().sum(1).sqrt().clamp(min=1e-6) >= 0.05)
        if mask is None:
            return torch.tensor(100.0 * int(hit.sum()) / hit.numel(), dtype=torch.float64)
        return torch.tensor(100.0 * int(hit[mask].sum()) / int(mask.sum()), dtype=torch.float64)

    def flow64(src, tgt, vm):
        """calculate_flow_error over the M * B images (utils.py:220-296) with the count + 1e-5 in float64: the reference forms it in
        fp32 whatever the inputs.  src, tgt [M, B, 2, H, W], vm [M, B, H, W] or None."""
        mask = ~torch.isinf(tgt[:, :, 0]) & ~torch.isinf(tgt[:, :, 1]) & (tgt[:, :, 0].abs() > 0) & (tgt[:, :, 1].abs() > 0)
        if vm is not None:
            mask = mask & vm
        cnt = mask.sum(dim=(2, 3)).double() + 1e-5                                         # [M, B]
        e = (tgt - src).square().sum(2).sqrt() * mask
        u, v, ug, vg = src[:, :, 0], src[:, :, 1], tgt[:, :, 0], tgt[:, :, 1]
        cos = (1.0 + u * ug + v * vg) / (torch.sqrt(1 + u * u + v * v) * torch.sqrt(1 + ug * ug + vg * vg))
        a = torch.acos(cos.clamp(-1, 1)) * mask
        epe = e.sum(dim=(2, 3)) / cnt
        errors = dict(TEPE=epe.mean(), T3PE=((e > 3).sum(dim=(2, 3)).double() / cnt).mean(), TAE=(a.sum(dim=(2, 3)) / cnt).mean() * (180.0 / np.pi))
        return errors, [epe[i].mean() for i in range(src.shape[0])]

    def chain(preds, gts, ts, valid, ev_repr, classes, exact=False):
        """validation_step from the predictions on (raft_spline.py:159-194): {name: (value or None, updated)} in the dtype of the
        inputs.  classes: also through the Metric classes, asserted equal.  exact (the float64 pass): the quotients the reference
        forms in fp32 whatever the inputs -- NPE's, and count + 1e-5 of calculate_flow_error -- come from npe64 / flow64."""
        out = {}
        M = len(preds)

        def same(a, b):
            return torch.equal(a, b) or (bool(torch.isnan(a)) and bool(torch.isnan(b)))

        def single(prefix, mask):
            try:
                row = [R.epe_masked(preds[-1], gts[-1], mask), R.ae_masked(preds[-1], gts[-1], mask)] + \
                      [R.n_pixel_error_masked(preds[-1], gts[-1], mask, k) for k in (1, 2, 3)]
                if exact:
                    row[2:] = [npe64(preds[-1], gts[-1], mask, k) for k in (1, 2, 3)]
            except AssertionError:                       # NPE on an empty mask (utils.py:199): nothing of this row is pinned
                assert mask is not None and int(mask.sum()) == 0
                row = [None] * 5
            for k, v in zip(SINGLE, row):
                out[prefix + k] = (v, 0 if v is None else 1)
            if classes and row[0] is not None:
                for k, met in zip(SINGLE, (R.EPE(), R.AE(degrees=True), R.NPE(1), R.NPE(2), R.NPE(3))):
                    met.update(preds[-1], gts[-1], mask)
                    assert same(met.compute(), out[prefix + k][0].float()), (prefix, k)

        def multi(prefix, masks):
            epe = R.epe_masked_multi(preds, gts, masks)
            out[prefix + 'epe_multi'] = (epe, 0 if epe is None else 1)
            out[prefix + 'ae_multi'] = (R.ae_masked_multi(preds, gts, masks, True), 1)
            src, tgt = torch.stack(preds), torch.stack(gts)                       # FLOW_METRICS_MULTI.update (utils.py:513-531)
            vm = torch.stack(masks) if masks is not None else None
            errors = R.calculate_trajectory_flow_error(tgt, src, vm)
            steps = [R.calculate_flow_error(tgt[i], src[i], vm[i][:, None] if vm is not None else None)['EPE'] for i in range(M)]
            if exact:
                errors, steps = flow64(src, tgt, vm)
            for k in ('T3PE', 'TEPE', 'TAE'):
                out[prefix + k] = (errors[k], 1)
            for i in range(M):
                out[f'{prefix}EPE_STEP{str(i).zfill(2)}'] = (steps[i], 1)
            if classes:
                for k, met in (('epe_multi', R.EPE_MULTI()), ('ae_multi', R.AE_MULTI(degrees=True))):
                    met.update(preds, gts, masks)
                    assert (int(met.total) == 0 and out[prefix + k][0] is None) or same(met.compute(), out[prefix + k][0].float()), (prefix, k)
                met = R.FLOW_METRICS_MULTI()
                met.update(preds, gts, masks)
                for k, v in met.compute().items():
                    assert same(v, out[prefix + k][0].float()), (prefix, k)

        single('val/', None)
        multi('val/', None)
        event_mask = torch.abs(ev_repr).any(dim=1) > 0                             # raft_spline.py:164
        single('val/masked_', event_mask)
        if valid is not None:
            masks_ev, masks = [event_mask & valid[:, s] for s in range(M)], [valid[:, s] for s in range(M)]
        else:
            masks_ev, masks = [event_mask for _ in range(M)], None
        multi('val/ev_masked_', masks_ev)
        multi('val/masked_', masks)
        lin = R.predictions_from_lin_assumption(preds[-1], ts)
        out['val/epe_multi_lin'] = (R.epe_masked_multi(lin, gts), 1)
        out['val/ae_multi_lin'] = (R.ae_masked_multi(lin, gts, None, True), 1)
        return out

    def curves64(P, Mk, times, scale):
        """The curves part by part in float64 (as formula64 of tools/gen_golden_cvx.py)."""
        import math
        P, Mk = P.double(), Mk.double()
        B, c2, h, w = P.shape
        d, H, W = c2 // 2, 8 * h, 8 * w
        y, x = torch.arange(H), torch.arange(W)
        cy, sy, cx, sx = (y // 8)[:, None], (y % 8)[:, None], (x // 8)[None, :], (x % 8)[None, :]
        logits = Mk.view(B, 9, 8, 8, h, w)[:, :, sy, sx, cy, cx]
        e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        wk = e / e.sum(dim=1, keepdim=True)
        P0 = torch.nn.functional.pad(P, (1, 1, 1, 1))
        up = 0
        for k in range(9):
            up = up + wk[:, None, k] * 8 * P0[:, :, cy + k // 3, cx + k % 3]
        bm = torch.tensor([[math.comb(d, i) * (1 - t) ** (d - i) * t ** i for i in range(1, d + 1)] for t in times], dtype=torch.float64).float()
        return torch.einsum('bcjhw,tj->tbchw', up.view(B, 2, d, H, W), bm.double()) * scale

    for idx, (name, B, d, hw, times, C, has_valid, scale, grid) in enumerate(CASES):
        gen = torch.Generator().manual_seed(1500 + idx)
        M = len(times)
        out = dict(times=np.asarray(times, dtype=np.float64), scale=np.float64(scale))
        if d:
            h, w = hw
            H, W = 8 * h, 8 * w
            P = torch.randn(B, 2 * d, h, w, generator=gen) * 0.5
            Mk = torch.round(torch.randn(B, 576, h, w, generator=gen) * 2.0 * 2.0) / 2.0
            curve = BezierCurves(P).create_upsampled(Mk)
            pred = torch.stack([curve.get_flow_from_reference(float(t)) * scale for t in times])      # raft_spline.py:133-138
            pred64 = curves64(P, Mk, times, scale)
            out.update(params=P.numpy(), mask=Mk.numpy())
        else:
            H, W = hw
            pred = torch.randn(M, B, 2, H, W, generator=gen) * 2.0
            pred64 = pred.double()
        # ground truth: the prediction plus an error of 0.02 .. 6 px in a random direction, on the grid; 6 % exactly zero vectors,
        # 6 % with exactly one zero component
        mag = torch.exp(torch.rand(B, M, H, W, generator=gen) * (np.log(6.0) - np.log(0.02)) + np.log(0.02))
        ang = torch.rand(B, M, H, W, generator=gen) * (2 * np.pi)
        gt = pred.permute(1, 0, 2, 3, 4) + torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=2)
        gt = torch.round(gt * grid) / grid
        kind = torch.rand(B, M, H, W, generator=gen)
        gt[:, :, 0][kind < 0.03] = 0.0
        gt[:, :, 1][(kind >= 0.03) & (kind < 0.06)] = 0.0
        gt[(kind >= 0.06)[:, :, None].expand_as(gt) & (kind < 0.12)[:, :, None].expand_as(gt)] = 0.0
        one_zero = ((gt[:, :, 0] == 0) ^ (gt[:, :, 1] == 0))
        for rounds in range(64):
            bad = violations(pred64, gt.double())
            if not bad.any():
                break
            gt[:, :, 0][bad & (gt[:, :, 0] != 0)] += 1.0 / 256
            gt[:, :, 1][bad & (gt[:, :, 0] == 0)] += 1.0 / 256
        assert not violations(pred64, gt.double()).any()
        assert int(one_zero.sum()) > 0 and int(((gt[:, :, 0] == 0) & (gt[:, :, 1] == 0)).sum()) > 0
        ev = torch.randn(B, C, H, W, generator=gen) * (torch.rand(B, C, H, W, generator=gen) < 0.15)
        ev = torch.round(ev * 16) / 16
        valid = None
        if has_valid:
            valid = torch.rand(B, M, H, W, generator=gen) < 0.7
        if name == 'a':
            ev[0, :, 3, 5] = 0.0
            ev[0, 2, 3, 5] = float('nan')                   # a NaN counts as an event (abs(NaN).any() is True)
        if name == 'c':
            valid[:, 2] = False                             # a step without a valid pixel: ae_multi is NaN, epe_multi skips the step
            few = torch.zeros(M, H, W, dtype=torch.bool)
            few[:, 5, 100:103] = True
            few[2] = False
            valid[1] = few                                  # a sample with three valid pixels per step: per-image and per-batch means differ
        if name == 'e':
            ev[:] = 0.0                                     # no event anywhere
        gts32 = [gt[:, m].contiguous() for m in range(M)]
        ts = [float(t) for t in times]
        ref = chain([p for p in pred], gts32, ts, valid, ev, classes=(M == 6))
        ts64 = [float(np.float32(t)) for t in times]        # the fp32 product of utils.py:73 rounds the factor
        f64 = chain([p for p in pred64], [g.double() for g in gts32], ts64, valid, ev.double(), classes=False, exact=True)
        keys = list(ref.keys())
        assert keys == list(f64.keys()) and len(keys) == 12 + 3 * (5 + M)
        r = np.array([np.nan if ref[k][0] is None else float(ref[k][0]) for k in keys], dtype=np.float32)
        f = np.array([np.nan if f64[k][0] is None else float(f64[k][0]) for k in keys], dtype=np.float64)
        upd = np.array([ref[k][1] for k in keys], dtype=np.int32)
        assert all(ref[k][0] is None or ref[k][0].dtype == torch.float32 for k in keys)
        assert all(f64[k][0] is None or f64[k][0].dtype == torch.float64 for k in keys)
        assert [ref[k][1] for k in keys] == [f64[k][1] for k in keys] and np.array_equal(np.isnan(r), np.isnan(f))
        err = np.where(np.isnan(f), 0.0, np.abs(r.astype(np.float64) - f))
        assert (err <= 1e-5 * np.maximum(np.abs(np.nan_to_num(f)), 1.0)).all(), 'the float64 chain left the reference'
        out.update(flow_gt=gt.numpy(), ev_repr=ev.numpy(), keys=np.array(keys), ref=r, updated=upd, f64=f, err=err)
        if valid is not None:
            out['flow_valid'] = valid.numpy()
        path = os.path.join(args.out, f'g15_val_{name}.npz')
        sizes = []
        if name == 'c':
            save_npz(os.path.join(args.out, f'g15_val_{name}_pred.npz'), dict(pred=pred.numpy()))
            sizes.append(os.path.getsize(os.path.join(args.out, f'g15_val_{name}_pred.npz')))
        else:
            out['pred'] = pred.numpy()
        save_npz(path, out)
        sizes.insert(0, os.path.getsize(path))
        rel = np.where(np.isnan(f) | (f == 0), 0.0, err / np.maximum(np.abs(f), 1e-300))
        print(f'g15_val_{name}: {sizes} B  {len(keys)} keys  {rounds} margin rounds  NaN keys {int(np.isnan(f).sum())}  '
              f'not updated {int((upd == 0).sum())}  max rel err {rel.max():.3g} ({keys[int(rel.argmax())]})')


if __name__ == '__main__':
    main()
