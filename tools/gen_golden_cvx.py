#!/usr/bin/env python3
"""Fixtures g13_cvx_<case>.npz for the RAFT-spline output head (utils.trajectories_from_bezier(..., up_mask=...),
utils.flows_from_bezier): the UNMODIFIED reference's `BezierCurves(params).create_upsampled(mask).get_flow_from_reference(times)`
(src/models/raft_spline/curves/base.py:35-38, 95-123; bezier.py:92-113; raft_spline/utils.py:30-45) in fp32, sampled at the tile
centres of the reference's get_optical_flow_tile_mask, beside a float64 evaluation of the same formula written out below, and
the measured distance between the two -- the tests derive their tolerances from it.

    python tools/gen_golden_cvx.py --ref PATH_TO_REFERENCE [--out tests/golden]

As oracle/gen_golden.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files
are imported as they are, and only DATA is written.  Deterministic (seeded, one thread): a second run reproduces the files bit
for bit.

Every file holds
  params [B, 2d, h, w], mask [B, 576, h, w], times [8], tile, scale, g [B, 8, n, 2] (the cotangent), flow_times (three indices)
  traj, flows, grad_params, grad_mask            the reference, fp32 (flows [3, B, 2, 8h, 8w] at times[flow_times])
  traj64, flows64, grad_params64, grad_mask64    the float64 evaluation
  err_traj, err_flows, err_grad_params, err_grad_mask     max |reference fp32 - float64|
The logits are drawn on a grid of 1/16 (times 30 in case c) and the float64 results keep 29 significant bits (2^-29 relative:
1/128 of the tolerance floor of the tests), so that the compressed files stay small; the errors are measured against the stored
values."""
import argparse
import math
import os
import sys

import numpy as np

TIMES = [0.41, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0, 1.0]          # t_ref, five bin mid-times, and the two ends base.py:102-106 special-cases
FLOW_TIMES = [0, 3, 7]
CASES = [  # name, B, d, (h, w), tile, scale, logit factor
    ('a', 2, 10, (2, 3), 4, 1.0, 1.0),
    ('b', 1, 3, (3, 5), 8, 1.0, 1.0),
    ('c', 2, 2, (3, 4), 2, 1.0, 30.0),
    ('d', 1, 16, (4, 4), 16, 1.0, 1.0),
    ('e', 1, 10, (3, 33), 4, 8.0, 1.0),
]


def keep29(a):
    """float64 array with the low 24 mantissa bits cleared."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return (a.view(np.int64) & ~np.int64((1 << 24) - 1)).view(np.float64)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'oracle', 'stubs'))
    sys.path.insert(1, args.ref)
    import torch
    from src.models.raft_spline.curves import BezierCurves          # reference, unmodified
    from src import utils as rutils                                 # reference, unmodified

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)
    times = np.asarray(TIMES, dtype='float64')

    def formula64(P, M, bm, pos, scale, g):
        """Part by part in float64: softmax over k of M[b, k, sy, sx, cy, cx]; up = sum_k w_k * 8 * P0[cy + k // 3 - 1, cx + k % 3 - 1];
        flow_t = scale * sum_j bm[t, j] up[j]; traj = pos + flow ((y, x) order)."""
        P = P.double().requires_grad_(True)
        M = M.double().requires_grad_(True)
        B, c2, h, w = P.shape
        d, H, W = c2 // 2, 8 * h, 8 * w
        y, x = torch.arange(H), torch.arange(W)
        cy, sy, cx, sx = (y // 8)[:, None], (y % 8)[:, None], (x // 8)[None, :], (x % 8)[None, :]
        logits = M.view(B, 9, 8, 8, h, w)[:, :, sy, sx, cy, cx]                      # [B, 9, H, W]
        e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        wk = e / e.sum(dim=1, keepdim=True)
        P0 = torch.cat((torch.zeros(B, c2, 1, w, dtype=torch.float64), P, torch.zeros(B, c2, 1, w, dtype=torch.float64)), dim=2)
        P0 = torch.cat((torch.zeros(B, c2, h + 2, 1, dtype=torch.float64), P0, torch.zeros(B, c2, h + 2, 1, dtype=torch.float64)), dim=3)
        up = 0
        for k in range(9):
            up = up + wk[:, None, k] * 8 * P0[:, :, cy + k // 3, cx + k % 3]         # [B, 2d, H, W]
        flows = torch.einsum('bcjhw,tj->tbchw', up.view(B, 2, d, H, W), bm.double()) * scale
        at = flows[:, :, :, pos[:, 0], pos[:, 1]]                                    # [T, B, 2, n]
        traj = torch.stack((at[:, :, 1], at[:, :, 0]), dim=-1).permute(1, 0, 2, 3) + pos.double()[None, None]
        gp, gm = torch.autograd.grad(traj, [P, M], g.double())
        return traj.detach(), flows.detach()[FLOW_TIMES], gp, gm

    def reference32(P, M, pos, scale, g):
        P = P.clone().requires_grad_(True)
        M = M.clone().requires_grad_(True)
        curve = BezierCurves(P).create_upsampled(M)
        flows = curve.get_flow_from_reference(times) * scale                          # [T, B, 2, H, W], (x, y)
        at = flows[:, :, :, pos[:, 0], pos[:, 1]]
        traj = torch.stack((at[:, :, 1], at[:, :, 0]), dim=-1).permute(1, 0, 2, 3) + pos.float()[None, None]
        gp, gm = torch.autograd.grad(traj, [P, M], g)
        return traj.detach(), flows.detach()[FLOW_TIMES], gp, gm

    for idx, (name, B, d, (h, w), tile, scale, lf) in enumerate(CASES):
        gen = torch.Generator().manual_seed(1300 + idx)
        P = torch.randn(B, 2 * d, h, w, generator=gen) * 0.5
        M = torch.round(torch.randn(B, 576, h, w, generator=gen) * 2.0 * 16.0) / 16.0 * lf
        pos = torch.nonzero(rutils.get_optical_flow_tile_mask((8 * h, 8 * w), tile))
        g = torch.randn(B, len(TIMES), pos.shape[0], 2, generator=gen)
        # the Bernstein matrix as bezier.py:102-107 builds it: float64, then fp32
        bm = torch.tensor([[math.comb(d, i) * (1 - t) ** (d - i) * t ** i for i in range(1, d + 1)] for t in TIMES], dtype=torch.float64).float()
        ref = [t.numpy() for t in reference32(P, M, pos, scale, g)]
        f64 = [keep29(t.numpy()) for t in formula64(P, M, bm, pos, scale, g)]
        names = ('traj', 'flows', 'grad_params', 'grad_mask')
        out = dict(params=P.numpy(), mask=M.numpy(), times=times, tile=np.int64(tile), scale=np.float64(scale), g=g.numpy(),
                   flow_times=np.asarray(FLOW_TIMES, dtype=np.int64))
        for nm, r, f in zip(names, ref, f64):
            assert r.dtype == np.float32 and r.shape == f.shape, (nm, r.dtype, r.shape, f.shape)
            out[nm], out[nm + '64'] = r, f
            out['err_' + nm] = np.float64(np.abs(r.astype(np.float64) - f).max())
        path = os.path.join(args.out, f'g13_cvx_{name}.npz')
        save_npz(path, out)
        nz = float((ref[3] != 0).mean())
        print(f'g13_cvx_{name}: {os.path.getsize(path)} B  n = {pos.shape[0]}  ' +
              '  '.join(f"err_{nm} = {out['err_' + nm]:.3g} (max {np.abs(f).max():.3g})" for nm, f in zip(names, f64)) +
              f'  grad_mask non-zero share {nz:.6f}')


if __name__ == '__main__':
    main()
