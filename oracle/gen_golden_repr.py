#!/usr/bin/env python3
"""Golden vectors for the centred voxel grid from the UNMODIFIED reference (src/loader/utils/representation.py imports only
torch; it sets torch's thread counts to 1 at import, so it is imported before anything else runs).

    python oracle/gen_golden_repr.py [--ref /root/reference] [--out tests/golden]

Only data goes into the files: inputs, shape, centres, the raw, the normalised and the resized grid."""
import argparse
import importlib.util
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location('ref_representation', os.path.join(args.ref, 'src/loader/utils/representation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from oracle.repr_oracle import synth_int_events

    def save(name, x, y, p, t, shape, centres, raw, normed=None, resized=None):
        d = dict(x=x.numpy(), y=y.numpy(), pol=p.numpy(), time=t.numpy(), shape=np.array(shape),
                 centres=np.array(centres if centres is not None else [], dtype=np.int64), raw=raw.numpy())
        if normed is not None:
            d['normed'] = normed.numpy()
        if resized is not None:
            d['resized'] = resized.numpy()
        np.savez_compressed(os.path.join(args.out, name + '.npz'), **d)
        print(name, tuple(raw.shape), float(raw.abs().sum()), None if normed is None else float(normed.abs().sum()))

    def run(shape, x, y, p, t, centres):
        vg = mod.VoxelGrid(*shape)
        raw = vg.convert(x, y, p, t) if centres is None else vg.convert(x, y, p, t, centres[0], centres[1])
        return raw, mod.norm_voxel_grid(raw.clone())

    # (a) integer xy, default centres
    shape = (5, 24, 32)
    x, y, p, t = synth_int_events(4000, shape, 0, 1000000, 11)
    raw, normed = run(shape, x, y, p, t, None)
    save('g12_repr_a_int_default', x, y, p, t, shape, None, raw, normed)
    # (b) integer xy, explicit centres, events of the extended window
    shape = (9, 24, 32)
    cen = (200000, 800000)
    t_lo, t_hi = mod.VoxelGrid(*shape).get_extended_time_window(*cen)
    x, y, p, t = synth_int_events(5000, shape, t_lo, t_hi, 12)
    raw, normed = run(shape, x, y, p, t, cen)
    save('g12_repr_b_int_centres', x, y, p, t, shape, cen, raw, normed)
    # (c) float xy with coordinates outside the sensor, explicit centres
    shape = (7, 20, 28)
    cen = (150000, 900000)
    t_lo, t_hi = mod.VoxelGrid(*shape).get_extended_time_window(*cen)
    x, y, p, t = synth_int_events(5000, shape, t_lo, t_hi, 13, float_xy=True)
    raw, _ = run(shape, x, y, p, t, cen)
    save('g12_repr_c_float_centres', x, y, p, t, shape, cen, raw)
    # (d) the EVIMO2 chain (datasubset.py:146-189): absolute microseconds, pol = 1 - p, 65 channels, normalised, resized
    shape = (65, 30, 40)
    x, y, p, t = synth_int_events(5000, shape, 41234567, 41234567 + 300000, 14)
    p = 1 - p
    raw, normed = run(shape, x, y, p, t, None)
    resized = F.interpolate(normed[None], size=(24, 32), mode='bilinear', align_corners=False)[0]
    save('g12_repr_d_evimo2_chain', x, y, p, t, shape, None, raw, normed, resized)
    # (e) degenerate normalisations
    shape = (5, 12, 16)
    cen = (1000, 5000)                                             # one channel per 1000 us
    i = torch.arange(20)
    x, y, p, t = (i % 16).int(), (i // 16 + 3).int(), torch.ones(20, dtype=torch.int64), torch.sort(1000 + 1000 * (i % 5)).values
    raw, normed = run(shape, x, y, p, t, cen)
    save('g12_repr_e1_std_zero', x, y, p, t, shape, cen, raw, normed)
    x, y, p, t = torch.tensor([7], dtype=torch.int32), torch.tensor([5], dtype=torch.int32), torch.tensor([1]), torch.tensor([3000])
    raw, normed = run(shape, x, y, p, t, cen)
    save('g12_repr_e2_single', x, y, p, t, shape, cen, raw, normed)
    x, y, p, t = torch.tensor([2, 9], dtype=torch.int32), torch.tensor([4, 8], dtype=torch.int32), torch.tensor([1, 0]), torch.tensor([500, 5500])
    raw, normed = run(shape, x, y, p, t, cen)
    save('g12_repr_e3_outside_centres', x, y, p, t, shape, cen, raw, normed)
    e = torch.zeros(0, dtype=torch.int32)
    x, y, p, t = e, e, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    raw, normed = run(shape, x, y, p, t, cen)
    save('g12_repr_e4_empty', x, y, p, t, shape, cen, raw, normed)


if __name__ == '__main__':
    main()
