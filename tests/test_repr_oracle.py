"""Centred voxel grid (EVIMO2 / MultiFlow network input): the CPU oracle against the reference's golden vectors, and the guard
on the inputs of the full-size GPU tests (tests/test_gpu_repr.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import repr_oracle as R

REPR_CASES = ['g12_repr_a_int_default', 'g12_repr_b_int_centres', 'g12_repr_c_float_centres', 'g12_repr_d_evimo2_chain',
              'g12_repr_e1_std_zero', 'g12_repr_e2_single', 'g12_repr_e3_outside_centres', 'g12_repr_e4_empty']
RESIZE_TO = {'g12_repr_d_evimo2_chain': (24, 32)}

# inputs of the full-size GPU tests: name -> (shape, float_xy, [(seed, events, centres or None, t range or None)])
T_EVIMO2 = (41234567, 41934567)
FULL_INPUTS = {
    'evimo2': ((65, 480, 640), False, [(3, 1500000, None, T_EVIMO2), (4, 800000, None, T_EVIMO2)]),
    'multiflow': ((65, 384, 512), False, [(3, 800000, (100000, 900000), None), (5, 600000, (250000, 900000), None)]),
    'float_xy': ((15, 120, 160), True, [(3, 200000, (100000, 900000), None)]),
}


def load_repr(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    g = {k: z[k] for k in z.files}
    g['shape'] = tuple(int(v) for v in g['shape'])
    g['centres'] = tuple(int(v) for v in g['centres']) if g['centres'].size else None
    return g


def full_sample(name, k):
    """(x, y, pol, time, centres) of sample k of a full-size case: explicit centres come with the extended window."""
    shape, float_xy, samples = FULL_INPUTS[name]
    seed, n, centres, t_range = samples[k]
    t_lo, t_hi = t_range if centres is None else R.extended_time_window(shape[0], *centres)
    x, y, p, t = R.synth_int_events(n, shape, t_lo, t_hi, seed, float_xy=float_xy)
    return x, y, p, t, centres


@pytest.mark.parametrize('name', REPR_CASES)
def test_repr_oracle_matches_reference(name):
    g = load_repr(name)
    x, y, p, t = (torch.from_numpy(g[k]) for k in ('x', 'y', 'pol', 'time'))
    c = g['centres'] or (None, None)
    raw = R.voxel_grid(x, y, p, t, g['shape'], *c)
    np.testing.assert_allclose(raw.numpy(), g['raw'], rtol=0, atol=1e-6)
    if 'normed' in g:
        normed = R.norm_voxel_grid(raw)
        np.testing.assert_allclose(normed.numpy(), g['normed'], rtol=0, atol=1e-6)
        if name.startswith('g12_repr_e') and name != 'g12_repr_e3_outside_centres':
            assert not g['normed'].any() and not normed.numpy().any()          # the degenerate branches end all zero
    if 'resized' in g:
        out = R.resize_bilinear(R.norm_voxel_grid(raw), RESIZE_TO[name])
        np.testing.assert_allclose(out.numpy(), g['resized'], rtol=0, atol=1e-6)


def test_repr_extended_window_and_generator():
    assert R.extended_time_window(9, 200000, 800000) == (125000, 875000)
    assert R.extended_time_window(65, 250000, 900000) == (239843, 910157)
    x, y, p, t = R.synth_int_events(1000, (5, 24, 32), 10, 99, 1)
    assert x.dtype == torch.int32 and t.dtype == torch.int64 and bool((t[1:] >= t[:-1]).all())
    assert int(t.min()) >= 10 and int(t.max()) <= 99 and set(p.tolist()) <= {0, 1}
    xf, yf, _, _ = R.synth_int_events(20000, (5, 24, 32), 10, 99, 1, float_xy=True)
    assert xf.dtype == torch.float32 and float(xf.min()) < 0 and float(yf.max()) > 23     # some fall outside the sensor


@pytest.mark.parametrize('name,k', [(n, k) for n, v in FULL_INPUTS.items() for k in range(len(v[2]))])
def test_repr_full_size_inputs_keep_the_reference_inside_the_cap(name, k):
    """The full-size GPU tests allow 2 entries per sample beyond 5e-6 * max(1, |ref|max): an entry that cancels to exactly zero
    in one summation order and not in another changes its non-zero status and with it its normalised value.  That allowance
    must not hide a failure, so for exactly those inputs the oracle's fp32 grid and the same taps summed in float64 must have
    NO entry of different zero / non-zero status and must differ by less than a third of the tolerance, raw and normalised."""
    shape = FULL_INPUTS[name][0]
    x, y, p, t, centres = full_sample(name, k)
    c = centres or (None, None)
    g32 = R.voxel_grid(x, y, p, t, shape, *c)
    g64 = R.voxel_grid(x, y, p, t, shape, *c, dtype=torch.float64)
    flips = int(((g32 != 0) != (g64 != 0)).sum())
    d_raw = float((g32.double() - g64).abs().max())
    tol_raw = 5e-6 * max(1.0, float(g32.abs().max()))
    n32, n64 = R.norm_voxel_grid(g32), R.norm_voxel_grid(g64)
    d_norm = float((n32.double() - n64).abs().max())
    tol_norm = 5e-6 * max(1.0, float(n32.abs().max()))
    print(f'{name}[{k}]: flips {flips}, raw {d_raw:.2e} (|max| {float(g32.abs().max()):.1f}), '
          f'normalised {d_norm:.2e} (|max| {float(n32.abs().max()):.1f})')
    assert flips == 0
    assert d_raw < tol_raw / 3 and d_norm < tol_norm / 3
