#!/usr/bin/env python3
"""Fixtures g16_corr_<case>.npz for the RAFT-spline correlation lookup (utils.corr_pyramid, utils.CorrLookup): the UNMODIFIED
reference's chain of raft.py:165-189 --

    block  = CorrBlockParallelMultiTarget(CorrComputation(fmap1, fmap2, num_levels), radius)      (corr.py:125-302)
    flows  = BezierCurves(params).get_flow_from_reference(times)                                   (base.py:95-123, bezier.py:92-113)
    out    = block(coords_grid(B, h, w) + flows)                                                   (corr.py:304-348, utils.py:4-28)

-- in fp32, beside a float64 evaluation of the lookup's formula written out below (sample position coords / 2^l + offset, bilinear,
zero padding per tap), and the measured distance between the two: the tests derive their tolerances from it.

    python tools/gen_golden_corr.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_cvx.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files are
imported as they are, and only DATA is written.  Deterministic (seeded, one thread): a second run reproduces the files bit for bit.

Every file holds
  fmap1 [B, D, h, w], fmap2 [n, B, D, h, w], num_levels [n], radius, params [B, 2d, h, w], times [n], g (the cotangent of out)
  level_sha_<l> [32] uint8           sha256 of the bytes of the reference's pyramid level l (fp32, C order); target_indices_<l>
  out, grad_coords, grad_params, grad_level_<l>           the reference, fp32 (every level a leaf of its own)
  out64, grad_coords64, grad_params64, grad_level_<l>64   the float64 evaluation (29 significant bits kept, as g13)
  err_<name>                         max |reference fp32 - float64|
The feature maps are drawn on a grid of 1/4 with D in {4, 16}: every product is a multiple of 1/16, sqrt(D) is a power of two and
the pools divide by 4, so every level is exact in fp32 whatever the summation order -- utils.corr_pyramid rebuilds the pyramid bit
for bit, and no volume is stored.  The control points of a pixel are redrawn while one of its coords / 2^l lies within 2^-10 of an
integer (the coordinate gradient has a kink there; the reference's own coordinate rounding is about 1e-6).  A case's seed is the first
of its series whose draw meets the conditions asserted below (zero share of `out`, windows inside level 0)."""
import argparse
import hashlib
import math
import os
import sys

import numpy as np

MARGIN = 2.0 ** -10
CASES = [  # name, B, D, (h, w), num_levels, d, radius, amplitude of the control points
    ('a', 2, 4, (6, 8), [1, 2], 3, 4, 3.0),           # every window is clipped
    ('b', 1, 16, (5, 7), [1, 1, 2], 10, 4, 3.0),      # odd sizes (the pool drops the last row and column); last time exactly 1.0
    ('c', 1, 4, (12, 14), [2, 1], 2, 4, 0.5),         # windows inside; level 1 holds target 0 only
    ('d', 2, 4, (4, 33), [2], 1, 2, 3.0),             # a row that ends inside a wave; r != 4
    ('e', 2, 4, (6, 8), [1, 2], 3, 4, 30.0),          # as a, control points x 10: nearly every window outside
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


def lookup_times(n):
    """(i + 1) / n: what raft.py:169-176 asks for with nbins_context = n + 1; the last is exactly 1.0."""
    return [(i + 1) / n for i in range(n)]


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
    from src.models.raft_spline.corr import CorrComputation, CorrBlockParallelMultiTarget       # reference, unmodified
    from src.models.raft_spline.curves import BezierCurves                                      # reference, unmodified
    from src.models.raft_spline.utils import coords_grid                                        # reference, unmodified

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)
    largest = max(os.path.getsize(os.path.join(args.out, f)) for f in os.listdir(args.out) if f.endswith('.npz') and not f.startswith('g16_corr_'))

    def bernstein(times, d):
        """The matrix of bezier.py:102-107: float64, then fp32."""
        return torch.tensor([[math.comb(d, i) * (1 - t) ** (d - i) * t ** i for i in range(1, d + 1)] for t in times], dtype=torch.float64).float()

    def centres64(P, bm):
        B, c2, h, w = P.shape
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        flows = torch.einsum('bcjhw,tj->tbchw', P.view(B, 2, c2 // 2, h, w), bm.double())
        return torch.stack((xs, ys), dim=0)[None, None] + flows                               # [T, B, 2, h, w], (x, y)

    def formula64(levels, tix, r, coords):
        """out[b, e * K * K + i * K + j, y, x] = bilinear sample of levels[l][k][b * h * w + y * w + x] at
        (coords[t, b, 0, y, x] / 2^l + j - r, coords[t, b, 1, y, x] / 2^l + i - r), zero outside, per tap."""
        T, B, _, h, w = coords.shape
        K = 2 * r + 1
        off = torch.arange(-r, r + 1, dtype=torch.float64)
        out = []
        for l, (lv, ts) in enumerate(zip(levels, tix)):
            hl, wl = lv.shape[-2:]
            for k, t in enumerate(ts):
                px = (coords[t, :, 0] / 2 ** l)[..., None, None] + off[None, None, None, None, :]          # [B, h, w, 1, K]
                py = (coords[t, :, 1] / 2 ** l)[..., None, None] + off[None, None, None, :, None]          # [B, h, w, K, 1]
                x0, y0 = torch.floor(px).detach(), torch.floor(py).detach()
                fx, fy = px - x0, py - y0
                vol = lv[k].reshape(B * h * w, hl * wl)

                def tap(yi, xi):
                    yi, xi = yi.expand(B, h, w, K, K), xi.expand(B, h, w, K, K)
                    ok = (yi >= 0) & (yi < hl) & (xi >= 0) & (xi < wl)
                    idx = (yi.clamp(0, hl - 1) * wl + xi.clamp(0, wl - 1)).long().reshape(B * h * w, K * K)
                    return vol.gather(1, idx).reshape(B, h, w, K, K) * ok
                val = (tap(y0, x0) * ((1 - fx) * (1 - fy)) + tap(y0, x0 + 1) * (fx * (1 - fy)) +
                       tap(y0 + 1, x0) * ((1 - fx) * fy) + tap(y0 + 1, x0 + 1) * (fx * fy))
                out.append(val.reshape(B, h, w, K * K).permute(0, 3, 1, 2))
        return torch.cat(out, dim=1)

    def draw(seed, B, D, h, w, nl, d, r, amp):
        gen = torch.Generator().manual_seed(seed)
        n = len(nl)
        f1 = torch.round(torch.randn(B, D, h, w, generator=gen) * 4.0) / 4.0
        f2 = torch.round(torch.randn(n, B, D, h, w, generator=gen) * 4.0) / 4.0
        P = torch.randn(B, 2 * d, h, w, generator=gen) * amp
        times = lookup_times(n)
        bm = bernstein(times, d)
        for _ in range(64):                                  # the margin at integers: redraw the control points of the pixels that miss it
            c = centres64(P.double(), bm)
            near = torch.zeros(B, h, w, dtype=torch.bool)
            for l in range(max(nl)):
                s = c / 2 ** l
                near |= ((s - torch.round(s)).abs() < 2 * MARGIN).any(dim=2).any(dim=0)
            if not bool(near.any()):
                break
            fresh = torch.randn(B, 2 * d, h, w, generator=gen) * amp
            P = torch.where(near[:, None], fresh, P)
        K = 2 * r + 1
        g = torch.randn(B, sum(1 for v in nl for _ in range(v)) * K * K, h, w, generator=gen)
        return f1, f2, P, times, bm, g

    for idx, (name, B, D, (h, w), nl, d, r, amp) in enumerate(CASES):
        for attempt in range(64):
            seed = 1600 + 100 * idx + attempt
            f1, f2, P, times, bm, g = draw(seed, B, D, h, w, nl, d, r, amp)
            # ---- the reference, fp32; every level a leaf of its own
            block = CorrBlockParallelMultiTarget(corr_computation_events=CorrComputation(f1, f2, num_levels_per_target=list(nl)), radius=r)
            tix = [cd.target_indices.tolist() for cd in block._corr_pyramid]
            levels32 = [cd.corr.detach().clone() for cd in block._corr_pyramid]
            leaves = [lv.clone().requires_grad_(True) for lv in levels32]
            for cd, lf in zip(block._corr_pyramid, leaves):
                cd._corr = lf
            Pr = P.clone().requires_grad_(True)
            coords1 = coords_grid(B, h, w, Pr.device) + BezierCurves(Pr).get_flow_from_reference(time=list(times))
            out = block(coords1)
            ref = [t.detach().numpy() for t in (out,) + torch.autograd.grad(out, [coords1, Pr] + leaves, g)]
            # ---- float64
            P64 = P.double().requires_grad_(True)
            lv64 = [lv.double().requires_grad_(True) for lv in levels32]
            c64 = centres64(P64, bm)
            out64 = formula64(lv64, tix, r, c64)
            f64 = [keep29(t.detach().numpy()) for t in (out64,) + torch.autograd.grad(out64, [c64, P64] + lv64, g.double())]
            # ---- what the case must reach
            c = c64.detach()
            margin = min(float(((c / 2 ** l) - torch.round(c / 2 ** l)).abs().min()) for l in range(max(nl)))
            c32 = coords1.detach().double()
            margin = min(margin, min(float(((c32 / 2 ** l) - torch.round(c32 / 2 ** l)).abs().min()) for l in range(max(nl))))
            zero = float((ref[0] == 0).mean())
            x0, y0 = torch.floor(c[:, :, 0]), torch.floor(c[:, :, 1])
            inside = float(((x0 - r >= 0) & (x0 + r + 1 <= w - 1) & (y0 - r >= 0) & (y0 + r + 1 <= h - 1)).double().mean())
            ok = margin >= MARGIN and (zero <= 0.75 if name != 'e' else 0.9 <= zero < 1.0) and (name != 'c' or inside >= 0.10)
            if ok:
                break
        assert margin >= MARGIN, (name, margin)
        if name == 'e':
            assert 0.9 <= zero < 1.0, (name, zero)
        else:
            assert zero <= 0.75, (name, zero)
        if name == 'c':
            assert inside >= 0.10, (name, inside)
            assert tix == [[0, 1], [0]], tix
        assert float(times[-1]) == 1.0
        for lv, lf in zip(levels32, lv64):                    # every level is exact: fp32 holds the float64 pyramid
            assert lv.dtype == torch.float32
        f1d, f2d = f1.double(), f2.double()
        lvl0 = (f1d.view(B, D, h * w).transpose(-1, -2) @ f2d.view(len(nl), B, D, h * w)) / math.sqrt(D)
        assert torch.equal(lvl0.view(levels32[0].shape), levels32[0].double()), name
        names = ['out', 'grad_coords', 'grad_params'] + [f'grad_level_{l}' for l in range(len(levels32))]
        arrays = dict(fmap1=f1.numpy(), fmap2=f2.numpy(), num_levels=np.asarray(nl, dtype=np.int64), radius=np.int64(r), params=P.numpy(),
                      times=np.asarray(times, dtype=np.float64), g=g.numpy(), seed=np.int64(seed))
        for l, lv in enumerate(levels32):
            arrays[f'level_sha_{l}'] = np.frombuffer(hashlib.sha256(lv.contiguous().numpy().tobytes()).digest(), dtype=np.uint8)
            arrays[f'target_indices_{l}'] = np.asarray(tix[l], dtype=np.int64)
        for nm, a32, a64 in zip(names, ref, f64):
            assert a32.dtype == np.float32 and a32.shape == a64.shape, (nm, a32.dtype, a32.shape, a64.shape)
            arrays[nm], arrays[nm + '64'] = a32, a64
            arrays['err_' + nm] = np.float64(np.abs(a32.astype(np.float64) - a64).max())
        path = os.path.join(args.out, f'g16_corr_{name}.npz')
        save_npz(path, arrays)
        if os.path.getsize(path) > largest:                   # only the float64 tensors then (err_X stays)
            for nm in names:
                del arrays[nm]
            save_npz(path, arrays)
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
        print(f'g16_corr_{name}: seed {seed}  {os.path.getsize(path)} B  zero share of out {zero:.3f}  windows inside level 0 {inside:.3f}  '
              f'margin {margin:.3g}  ' + '  '.join(f"err_{nm} = {arrays['err_' + nm]:.3g} (max {np.abs(a).max():.3g})" for nm, a in zip(names, f64)))


if __name__ == '__main__':
    main()
