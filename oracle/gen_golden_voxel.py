#!/usr/bin/env python3
"""Golden vectors for the voxel-grid builder from the UNMODIFIED reference
(src/loader/dsec/utils.py imports only torch and numpy, so no stand-ins are needed).

    python oracle/gen_golden_voxel.py [--ref /root/reference] [--out tests/golden]"""
import argparse
import importlib.util
import os
import sys

import numpy as np


def edge_cases(torch):
    """The g8_voxel_e* inputs: windows at the edges of the operation (tests/test_voxel_cases_host.py, tests/test_gpu_voxel_cases.py)."""
    from oracle.voxel_oracle import synth_raw_events
    f = lambda *v: torch.tensor(v, dtype=torch.float32)           # noqa: E731
    g = torch.Generator().manual_seed(9)
    n = 600
    xi, yi = torch.randint(0, 12, (n,), generator=g).float(), torch.randint(0, 10, (n,), generator=g).float()
    ti = torch.sort(torch.randint(0, 3, (n,), generator=g).float() / 2).values
    ti[0], ti[-1] = 0.0, 1.0
    pi = (torch.rand(n, generator=g) > 0.5).float()
    return (
        # a single event: t[-1] == t[0], t_norm is 0 / 0, every tap is masked out
        ('g8_voxel_e_single', (3, 6, 8), 'mean_std', 0, (f(2.5), f(3.25), f(0.4), f(1))),
        # three events at one time
        ('g8_voxel_e_equal_t', (3, 6, 8), 'max', 0, (f(2.5, 4.75, 1.25), f(3.25, 1.5, 2.0), f(0.5, 0.5, 0.5), f(1, 0, 1))),
        # times before t[0] and after t[-1], unsorted: channel sums 1.6, -0.4, 1.4
        ('g8_voxel_e_time', (3, 5, 6), None, 0, (f(2.5, 2.5, 2.5, 2.5), f(2.5, 2.5, 2.5, 2.5), f(0, -0.2, 1.3, 1), f(1, 1, 1, 1))),
        # a sparse window: the 0.9 quantile of |grid| is 0, every entry is clipped to +-0
        ('g8_voxel_e_sparse_q10', (5, 24, 32), 'mean_std', 0.1, synth_raw_events(40, (5, 24, 32), 7)),
        # two integer-coordinate events in channels 0 and C - 1: both entries 1, std 0, only the mean is subtracted
        ('g8_voxel_e_two_int', (4, 6, 8), 'mean_std', 0, (f(2, 5), f(3, 1), f(0, 1), f(1, 1))),
        # integer coordinates and channel times: +-1 votes, the threshold falls on a tie
        ('g8_voxel_e_int_q05', (3, 10, 12), None, 0.05, (xi, yi, ti, pi)),
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location('ref_dsec_utils', os.path.join(args.ref, 'src/loader/dsec/utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from oracle.voxel_oracle import synth_raw_events
    for name, shape, n, norm, seed, quant in (('g8_voxel_meanstd', (5, 24, 32), 4000, 'mean_std', 1, 0),
                                               ('g8_voxel_max', (3, 20, 28), 1500, 'max', 2, 0),
                                               ('g8_voxel_raw', (15, 30, 40), 6000, None, 3, 0),
                                               ('g8_voxel_q05_meanstd', (5, 24, 32), 9000, 'mean_std', 4, 0.05),
                                               ('g8_voxel_q10_raw', (3, 20, 28), 5000, None, 5, 0.1),
                                               ('g8_voxel_q02_max', (4, 22, 30), 12000, 'max', 6, 0.02)):
        x, y, t, p = synth_raw_events(n, shape, seed)
        vg = mod.VoxelGrid(shape, norm_type=norm, quantile=quant)
        out = vg.convert({'p': p, 't': t, 'x': x, 'y': y})
        np.savez_compressed(os.path.join(args.out, name + '.npz'), x=x.numpy(), y=y.numpy(), t=t.numpy(),
                            p=p.numpy(), shape=np.array(shape), norm=str(norm), quantile=np.float64(quant), grid=out.numpy())
        print(name, tuple(out.shape), float(out.abs().sum()))
    for name, shape, norm, quant, (x, y, t, p) in edge_cases(torch):
        vg = mod.VoxelGrid(shape, norm_type=norm, quantile=quant)
        out = vg.convert({'p': p, 't': t, 'x': x, 'y': y})
        np.savez_compressed(os.path.join(args.out, name + '.npz'), x=x.numpy(), y=y.numpy(), t=t.numpy(),
                            p=p.numpy(), shape=np.array(shape), norm=str(norm), quantile=np.float64(quant), grid=out.numpy())
        print(name, tuple(out.shape), float(out.abs().sum()), [float(v) for v in out.sum((1, 2))])


if __name__ == '__main__':
    main()
