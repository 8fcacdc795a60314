#!/usr/bin/env python3
"""Fixtures g23_corr_multi_<case>.npz for the events-plus-frames correlation pyramid (utils.corr_pyramid in list form,
utils.CorrLookup.from_fmaps): the UNMODIFIED reference's merge of raft.py:131-144 --

    block = CorrBlockParallelMultiTarget(corr_computation_events=CorrComputation(fmap1_events, fmap2_events, levels_events),
                                         corr_computation_frames=CorrComputation(fmap1_frames, fmap2_frames, levels_frames), radius)
    (corr.py:221-225 CorrComputation.__add__, 246-260 _corr_dot_prod_M_to_N, 282-302 the pooled levels, 304-348 the lookup)

-- in fp32.

    python tools/gen_golden_corr_multi.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_corr.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files are
imported as they are, and only DATA is written.  Deterministic (seeded, one thread): a second run reproduces the files bit for bit.

Every file holds
  fmap1_events [B, D, h, w], fmap2_events [n_e, B, D, h, w], fmap1_frames, fmap2_frames [n_f, B, D, h, w]
  num_levels_events [n_e], num_levels_frames [n_f], radius
  level_<l> [n_l, B*h*w, 1, h_l, w_l], target_indices_<l>     block._corr_pyramid, every level
  cot_<l>                                                     integer cotangents in [-1, 1] on the levels
  grad_fmap1_events, grad_fmap2_events, grad_fmap1_frames, grad_fmap2_frames     the reference's autograd gradients for them
  coords [T, B, 2, h, w], out [B, E * K * K, h, w]            block(coords), one coordinate set
  err_out                                                     max |out - the float64 evaluation of the lookup's formula|
The feature maps are drawn on a grid of 1/4 with D in {4, 16}, as in g16: every product is a multiple of 1/16, sqrt(D) is a power of
two and the pools divide by 4, so every level and every gradient is exact in fp32 whatever the summation order.  Asserted below: the
same chain in float64 gives the same numbers.  The coordinates are odd multiples of 1/16: no coords / 2^l lies within 1/64 of an
integer (the coordinate rounding of the reference's grid_sample is about 1e-6)."""
import argparse
import os
import sys

import numpy as np

CASES = [  # name, B, D, (h, w), level counts of the events, of the frames, radius
    ('a', 2, 16, (8, 12), [1, 2, 3], [3], 2),
    ('b', 1, 4, (8, 8), [1, 1], [2], 2),              # a reference that stops at level 0 beside one that goes deeper
]


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
    from src.models.raft_spline.corr import CorrComputation, CorrBlockParallelMultiTarget       # reference, unmodified
    from src.models.raft_spline.utils import coords_grid                                        # reference, unmodified

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)
    largest = max(os.path.getsize(os.path.join(args.out, f)) for f in os.listdir(args.out) if f.startswith('g16_corr_') and f.endswith('.npz'))

    def formula64(levels, tix, r, coords):
        """out[b, e * K * K + i * K + j, y, x] = bilinear sample of levels[l][k][b * h * w + y * w + x] at
        (coords[t, b, 0, y, x] / 2^l + j - r, coords[t, b, 1, y, x] / 2^l + i - r), zero outside, per tap (as tools/gen_golden_corr.py)."""
        T, B, _, h, w = coords.shape
        K = 2 * r + 1
        off = torch.arange(-r, r + 1, dtype=torch.float64)
        out = []
        for l, (lv, ts) in enumerate(zip(levels, tix)):
            hl, wl = lv.shape[-2:]
            for k, t in enumerate(ts):
                px = (coords[t, :, 0] / 2 ** l)[..., None, None] + off[None, None, None, None, :]
                py = (coords[t, :, 1] / 2 ** l)[..., None, None] + off[None, None, None, :, None]
                x0, y0 = torch.floor(px), torch.floor(py)
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

    def chain(maps, nle, nlf, r, cots):
        """The reference's merge over four leaves of the maps' dtype -> (block, levels, target indices, gradients to the leaves)."""
        leaves = [m.clone().requires_grad_(True) for m in maps]
        block = CorrBlockParallelMultiTarget(corr_computation_events=CorrComputation(leaves[0], leaves[1], num_levels_per_target=list(nle)),
                                             corr_computation_frames=CorrComputation(leaves[2], leaves[3], num_levels_per_target=list(nlf)),
                                             radius=r)
        levels = [cd.corr for cd in block._corr_pyramid]
        tix = [cd.target_indices.tolist() for cd in block._corr_pyramid]
        grads = torch.autograd.grad(levels, leaves, [c.to(levels[0].dtype) for c in cots]) if cots is not None else None
        return block, levels, tix, grads

    for idx, (name, B, D, (h, w), nle, nlf, r) in enumerate(CASES):
        seed = 2300 + 100 * idx
        gen = torch.Generator().manual_seed(seed)
        shapes = [(B, D, h, w), (len(nle), B, D, h, w), (B, D, h, w), (len(nlf), B, D, h, w)]
        maps = [torch.round(torch.randn(s, generator=gen) * 4.0) / 4.0 for s in shapes]
        nl = list(nle) + list(nlf)
        T = len(nl)
        want_tix = [[t for t, v in enumerate(nl) if v >= l + 1] for l in range(max(nl))]
        cots = [torch.randint(-1, 2, (len(ts), B * h * w, 1, h >> l, w >> l), generator=gen).float() for l, ts in enumerate(want_tix)]
        # odd multiples of 1/16 within about 3 pixels of the pixel's own position
        coords = coords_grid(B, h, w, 'cpu')[None] + (torch.randint(-24, 24, (T, B, 2, h, w), generator=gen).float() * 2 + 1) / 16
        # ---- the reference, fp32
        block, levels, tix, grads = chain(maps, nle, nlf, r, cots)
        assert tix == want_tix, (tix, want_tix)
        assert all(t.dtype == torch.float32 for t in levels + list(grads))
        with torch.no_grad():
            out = block(coords)
        # ---- the same chain in float64: every level and every gradient is exact in fp32
        _, levels64, _, grads64 = chain([m.double() for m in maps], nle, nlf, r, cots)
        for a, b in zip(levels + list(grads), levels64 + list(grads64)):
            assert b.dtype == torch.float64 and torch.equal(a.double(), b), name
        assert all(float(g.abs().max()) > 0 for g in grads)
        out64 = formula64([lv.detach() for lv in levels64], tix, r, coords.double())
        err_out = float((out.double() - out64).abs().max())
        arrays = dict(fmap1_events=maps[0].numpy(), fmap2_events=maps[1].numpy(), fmap1_frames=maps[2].numpy(), fmap2_frames=maps[3].numpy(),
                      num_levels_events=np.asarray(nle, dtype=np.int64), num_levels_frames=np.asarray(nlf, dtype=np.int64),
                      radius=np.int64(r), seed=np.int64(seed), coords=coords.numpy(), out=out.numpy(), err_out=np.float64(err_out))
        for l, lv in enumerate(levels):
            arrays[f'level_{l}'] = lv.detach().numpy()
            arrays[f'target_indices_{l}'] = np.asarray(tix[l], dtype=np.int64)
            arrays[f'cot_{l}'] = cots[l].numpy()
        for nm, g in zip(('grad_fmap1_events', 'grad_fmap2_events', 'grad_fmap1_frames', 'grad_fmap2_frames'), grads):
            arrays[nm] = g.numpy()
        path = os.path.join(args.out, f'g23_corr_multi_{name}.npz')
        save_npz(path, arrays)
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
        print(f'g23_corr_multi_{name}: seed {seed}  {os.path.getsize(path)} B (largest g16_corr: {largest})  levels {[tuple(lv.shape) for lv in levels]}  '
              f'err_out = {err_out:.3g} (max |out| {float(out.abs().max()):.3g})  zero share of out {float((out == 0).float().mean()):.3f}')


if __name__ == '__main__':
    main()
