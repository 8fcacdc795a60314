"""The voxel-grid edge cases on the CPU: both oracles against the reference's fixtures (the g8_voxel_e* edge windows included), the
float64 oracle against the pinned fp32 one, the route every case of tests/voxel_cases.py claims (from its geometry and its
per-bucket fills), the restated geometry against the library's own workspace size, and the two caps on the inputs."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_cases as VC
from oracle import voxel_oracle as V


@pytest.mark.parametrize('name', VC.BASE_FIXTURES + VC.EDGE_FIXTURES)
def test_both_oracles_match_the_reference(name):
    g, ev, shape, norm, q = VC.fixture(name)
    ref = torch.from_numpy(g['grid'])
    o32 = V.voxel_grid(*ev, shape, norm, q)
    o64 = V.voxel_grid64(*ev, shape, norm, q)[0]
    assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o64).all())
    np.testing.assert_allclose(o32.numpy(), g['grid'], rtol=0, atol=1e-6)
    # the reference is an fp32 computation: the float64 oracle is as far from it as fp32 rounding puts it
    tol = 4e-6 * max(1.0, float(ref.abs().max()))
    assert float((o64 - ref.double()).abs().max()) <= tol
    assert int(((o64 != 0) != (ref != 0)).sum()) == 0


def test_edge_fixtures_say_what_they_claim():
    for name in ('g8_voxel_e_single', 'g8_voxel_e_equal_t', 'g8_voxel_e_sparse_q10', 'g8_voxel_e_two_int'):
        grid = VC.fixture(name)[0]['grid']
        assert np.isfinite(grid).all() and not grid.any(), name
    g, ev, shape, norm, q = VC.fixture('g8_voxel_e_time')
    np.testing.assert_allclose(g['grid'].sum((1, 2)), [1.6, -0.4, 1.4], atol=1e-6)
    np.testing.assert_allclose(V.voxel_grid64(*ev, shape, norm, q)[0].sum((1, 2)).numpy(), [1.6, -0.4, 1.4], atol=1e-6)
    # sparse: the raw grid is not empty, its 0.9 quantile is 0
    g, ev, shape, norm, q = VC.fixture('g8_voxel_e_sparse_q10')
    raw = V.voxel_grid64(*ev, shape, None, 0.0)[0]
    assert int((raw != 0).sum()) > 100 and float(torch.quantile(raw.abs().float().view(-1), 0.9)) == 0.0
    # two integer events: the raw entries are exactly 1 in channels 0 and C - 1
    g, ev, shape, norm, q = VC.fixture('g8_voxel_e_two_int')
    raw = V.voxel_grid64(*ev, shape, None, 0.0)[0]
    assert raw[0, 3, 2] == 1 and raw[3, 1, 5] == 1 and float(raw.abs().sum()) == 2
    # tied threshold: the values at the two ranks and the one after them are equal
    g, ev, shape, norm, q = VC.fixture('g8_voxel_e_int_q05')
    srt = torch.sort(V.voxel_grid64(*ev, shape, None, 0.0)[0].abs().view(-1)).values
    pos = float(np.float32(1 - q) * np.float32(srt.numel() - 1))
    k0, k1 = int(np.floor(pos)), int(np.ceil(pos))
    assert k1 > k0 and srt[k0] == srt[k1] == srt[k1 + 1] and srt[k0] > 0 and srt[-1] > srt[k0]


@pytest.mark.parametrize('name', VC.CASE_NAMES)
def test_geometry_predicts_the_workspace(name):
    """vox_geometry must not drift from vox_layout / sb_layout: mpc_voxel_workspace_bytes is host-only."""
    from motionpriorcmax_amd import _lib as C
    c = VC.cases()[name]
    Cn, H, W = c.shape
    for B, N in ((c.B, c.N), (1, c.N), (3, 2 * c.N + 1), (2, 0)):
        s = C.VoxShape(B=B, N=N, C=Cn, H=H, W=W, norm=0, quantile=0.0, keep=0.0)
        assert int(C.lib().mpc_voxel_workspace_bytes(ctypes.byref(s))) == VC.vox_geometry(c.shape, N, B)['ws'], (B, N)


def test_cases_reach_their_routes():
    cs = VC.cases()
    # spill: both samples, two buckets each beyond the capacity, every record in the middle strip
    c = cs['spill']
    g = c.geometry()
    assert (g['SR'], g['NS'], g['nloc'], g['cap']) == (4, 3, 15, 4096) and c.B == 2
    for b in range(2):
        f = c.fills(b)
        print('spill fills', b, f.tolist())
        assert int((f > g['cap']).sum()) == 2 and int(f[1, 1]) > 5900 and int(f[2, 1]) > 5900 and int(f[:, [0, 2]].sum()) == 0
        x, y, t, p = c.samples[b]
        tn = 4 * (t - t[0]) / (t[-1] - t[0])
        assert bool(((tn[1:-1] > 1) & (tn[1:-1] < 2)).all()) and float(tn[0]) == 0 and float(tn[-1]) == 4
    # short last strip: rows 4 / 4 / 2, and events on both seams
    c = cs['short_strip']
    g = c.geometry()
    assert (g['SR'], g['NS']) == (4, 3) and c.shape[1] - 2 * g['SR'] == 2
    y0 = c.samples[0][1].int()
    assert int((y0 == 3).sum()) >= 500 and int((y0 == 7).sum()) >= 500 and int((y0 == 9).sum()) >= 300
    assert int(c.fills(0).max()) <= g['cap'] and int(c.fills(0).min()) > 0
    # wide: the 150 KB fallback
    c = cs['wide']
    g = c.geometry()
    assert VC.VOX_STRIP_KB * 1024 // (c.shape[2] * 8) == 0 and (g['SR'], g['NS'], g['lds']) == (1, 3, 96000)
    # tiny: an integer rank at (3, 5, 7) with q = 0.125
    pos = np.float32(1 - 0.125) * np.float32(3 * 5 * 7 - 1)
    assert float(pos) == 91.0
    assert cs['tiny_1x1x1'].samples[0][0].numel() == 2 and cs['tiny_3x5x7'].samples[0][0].numel() == 300
    # integer ties: a handful of magnitudes, many entries that were hit and cancel, tied thresholds
    c = cs['integer_ties']
    raw, taps = VC.expected('integer_ties', None, 0.0)[0]['raw64'], VC.expected('integer_ties', None, 0.0)[0]['taps']
    mags = torch.unique(raw.abs())
    cancelled = int(((raw == 0) & (taps > 0)).sum())
    print('integer ties: magnitudes', mags.tolist(), 'zero entries', int((raw == 0).sum()), 'of them hit', cancelled)
    assert mags.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and int((raw == 0).sum()) == 2047 and cancelled > 300
    thr = [float(torch.quantile(raw.abs().float().view(-1), 1 - q)) for q in (0.02, 0.05, 0.1, 0.14)]
    assert thr == [2.0, 2.0, 1.0, 1.0], thr
    # sparse: the threshold is 0 on a grid that is not empty; everything is clipped to +-0
    raw = VC.expected('sparse', None, 0.0)[0]['raw64']
    assert int((raw != 0).sum()) > 200 and float(torch.quantile(raw.abs().float().view(-1), 0.9)) == 0.0
    for nm in VC.NORMS:
        assert not VC.expected('sparse', nm, 0.1)[0]['g64'].any()
    # time: unsorted, before the first and after the last, a negative weight on channel 1 from -1 < t_norm < 0
    x, y, t, p = cs['time'].samples[0]
    tn = 3 * (t - t[0]) / (t[-1] - t[0])
    assert bool((t[1:] < t[:-1]).any()) and float(tn.min()) < -1 and float(tn.max()) > 4 and int(((tn > -1) & (tn < 0)).sum()) > 5
    # ragged
    c = cs['ragged']
    assert c.counts == [0, c.N, 1, c.N + 5] and c.B == 4
    assert not VC.expected('ragged', 'mean_std', 0.0)[0]['g64'].any() and not VC.expected('ragged', 'mean_std', 0.0)[2]['g64'].any()
    # non-finite: the bad rows are in the middle and the expectation has none of them
    c = cs['nonfinite']
    x, y = c.samples[0][0], c.samples[0][1]
    badrows = ~(torch.isfinite(x) & torch.isfinite(y) & (x.abs() < 1e9) & (y.abs() < 1e9) & (x > -8) & (y > -8) & (x < c.shape[2] + 8) & (y < c.shape[1] + 8))
    assert int(badrows.sum()) == 15 and not bool(badrows[0]) and not bool(badrows[-1])
    assert c.expect[0][0].numel() == x.numel() - 15 and bool(torch.isfinite(torch.stack(c.expect[0])).all())
    # zero span: NaN at the ends, both infinities between, and zeros from both oracles
    x, y, t, p = cs['zero_span'].samples[0]
    tn = 2 * (t - t[0]) / (t[-1] - t[0])
    assert bool(torch.isnan(tn[0])) and bool(torch.isnan(tn[-1])) and float(tn[1]) == float('-inf') and float(tn[2]) == float('inf')
    for nm in VC.NORMS:
        o = VC.expected('zero_span', nm, 0.0)[0]
        assert not o['g64'].any() and not o['g32'].any() and bool(torch.isfinite(o['g32']).all())
    # all equal: 40 equal entries in the last channel, the fp32 std is exactly 0, the output at most 2e-6
    o = VC.expected('all_equal', 'mean_std', 0.0)[0]
    nz = o['raw32'] != 0
    assert int(nz.sum()) == 40 and bool(nz[4].sum() == 40) and float(o['raw32'][nz].std()) == 0.0
    assert abs(float(o['raw32'][nz][0]) - 0.3) < 1e-6
    assert float(o['g32'].abs().max()) <= 2e-6 and float(o['g64'].abs().max()) <= 2e-6


@pytest.mark.parametrize('name,norm,q', VC.case_params())
def test_caps_and_oracle_distance(name, norm, q):
    """Cap 1 on the inputs (no entry within the raw bound of 0, fp32 and fp64 agree on the non-zero entries), the fp32 oracle
    finite and close to the float64 one: err32, which sets the bound on the device, is itself bounded by fp32 rounding of the sums
    -- 2^-22 per tap of the largest entry, times the multiplier."""
    for b, o in enumerate(VC.expected(name, norm, q)):
        tiny, flips = VC.input_caps(o)
        bound, err32, T = VC.bound_of(o)
        print(f'{name} {norm} q={q} sample {b}: err32 {err32:.3e} bound {bound:.3e} T {T} m {o["m"]:.4g} '
              f'entries within the raw bound of 0: {tiny}, non-zero flips: {flips}')
        assert tiny == 0 and flips == 0
        assert bool(torch.isfinite(o['g32']).all()) and bool(torch.isfinite(o['g64']).all())
        assert int(((o['g64'] != 0) != (o['g32'] != 0)).sum()) == 0
        assert err32 <= 2.0 ** -22 * max(T, 1) * max(float(o['raw64'].abs().max()), 1.0) * max(o['m'], 1.0) * 4
