"""CPU checks of tests/event_cases.py: the float64 reference agrees with the oracle and its autograd, a float32 stand-in of the kernel
arithmetic (Q33.30 truncation included) passes every case under the comparator, nine broken variants of it each fail the cases
named for them, and the generator is deterministic and puts into every case the edge it is named for."""
import numpy as np
import pytest
import torch

import event_cases as E
from oracle import focus_oracle as O


def _generic(split, scale_dt, T):
    """synth_events on 48 x 64 with a random LUT: nothing sits on an edge."""
    H, W, sp, nb, B, M = 48, 64, 4, 3, 2, 1500
    ev, num_pos = O.synth_events(B, M, (H, W), nb, seed=5, pad_frac=0.1)
    rng = np.random.default_rng(3)
    hq, wq = H // sp, W // sp
    ev = ev.numpy().copy()
    ev[..., 5] *= rng.uniform(0.3, 1.4, ev.shape[:2]).astype(np.float32)
    return E.Case(name='generic', H=H, W=W, sp=sp, nb=nb, T=T, B=B, split=split, scale_dt=scale_dt, mask=True,
                  num_pos=num_pos if split else M, ev=ev, kind=np.ones((B, M), dtype=np.int64), kinds=['pad', 'synth'],
                  lut=(2.5 * rng.standard_normal((B, nb, hq, wq, T, 2))).astype(np.float32),
                  gimg=rng.standard_normal((B * T, 2 if split else 1, H, W)).astype(np.float32),
                  add=rng.standard_normal((B, nb, hq, wq, T, 2)).astype(np.float32),
                  t_ref=np.array([E.T_REF], dtype=np.float32) if T == 1 else np.linspace(0, 1, T).astype(np.float32))


@pytest.mark.parametrize('split,scale_dt,T', [(True, True, 1), (False, False, 3)])
def test_reference_agrees_with_the_oracle_and_its_autograd(split, scale_dt, T):
    """The oracle works in fp32 and sums with scatter_add / index_put in an order of its own: it is held to the bound of the
    global-atomic kernels (gamma(n - 1 + N) of the absolute sum), with N_ORACLE roundings per event for its autograd."""
    c = _generic(split, scale_dt, T)
    cfg = dict(image_shape=(c.H, c.W), num_tref=T, num_bins=c.nb, num_knn=4, smooth_weight=0.0, lut_superpixel_size=c.sp,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=scale_dt, mask_image_border=True,
               polarity_aware_batching=split, interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    lut = torch.from_numpy(c.lut).clone().requires_grad_(True)
    _, _, raw = O.FocusLossOracle(**cfg).event_path(torch.from_numpy(c.ev), lut, torch.from_numpy(c.t_ref), c.num_pos)
    f = E.reference_fwd(c)
    assert float(f['mass'].sum()) > 100.0
    E.check('generic', f'oracle fwd T={T}', raw.detach().numpy(), f['ref'], f['allow_atomic'], c, f['prov'])
    (raw.reshape(c.gimg.shape) * torch.from_numpy(c.gimg)).sum().backward()
    b = E.reference_bwd(c, add=False, gcoef=1.0, gout=1.0, extra=E.N_ORACLE - E.N_G)
    assert int((b['n'] > 0).sum()) > 100
    E.check('generic', f'oracle bwd T={T}', lut.grad.numpy(), b['ref'], b['allow_atomic'], c, b['prov'])


@pytest.mark.parametrize('name', sorted(E.CASES))
def test_stand_in_passes_every_case(name):
    c = E.case(name)
    f = E.expected_fwd(name)
    E.check(name, 'stand-in fwd', E.standin_fwd(c), f['ref'], f['allow'], c, f['prov'])
    E.check(name, 'stand-in fwd fixed', E.standin_fwd(c, fixed=True).astype(np.float64) * E.Q30, f['ref'], f['allow_fixed'], c, f['prov'])
    for add in (False, True):
        b = E.expected_bwd(name, add)
        E.check(name, f'stand-in bwd add={add}', E.standin_bwd(c, add=add), b['ref'], b['allow'], c, b['prov'])
    # the tiled bounds are the tighter ones wherever more than one contribution meets
    assert bool((f['allow_atomic'][f['n'] > 32] > f['allow_fixed'][f['n'] > 32]).all())


@pytest.mark.parametrize('name', E.SPLAT_CASES)
@pytest.mark.parametrize('unit', [False, True])
def test_stand_in_passes_the_imager_rows(name, unit):
    s = E.splat_rows(name)
    f = E.reference_fwd(s, no_warp=True, unit_weight=unit)
    assert float(f['mass'].sum()) > 10.0
    E.check(name, f'stand-in splat unit={unit}', E.standin_fwd(s, no_warp=True, unit_weight=unit), f['ref'], f['allow'], s, f['prov'])


@pytest.mark.parametrize('mutant', E.MUTANTS)
def test_every_mutant_fails_the_cases_named_for_it(mutant):
    direction, names = E.CATCHES[mutant]
    for name in names:
        c = E.case(name)
        if direction == 'fwd':
            f = E.expected_fwd(name)
            r = E.compare(E.standin_fwd(c, mutant=mutant), f['ref'], f['allow'], c, f['prov'])
        else:
            b = E.expected_bwd(name, True)
            r = E.compare(E.standin_bwd(c, add=True, mutant=mutant), b['ref'], b['allow'], c, b['prov'])
        print(f'{mutant} on {name}: ratio {r.ratio:.3g} at {r.index}, touched by {r.provenance}')
        assert r.ratio > 1.0, (mutant, name, r)


def test_every_mutant_is_listed_and_every_case_has_its_rows():
    assert set(E.CATCHES) == set(E.MUTANTS) and len(E.MUTANTS) >= 7
    assert set(E.REQUIRED) == set(E.CASES)
    for name in E.CASES:
        c = E.case(name)
        for kind in E.REQUIRED[name]:
            assert c.count(kind) > 0, (name, kind)
        pad = c.kind == 0
        assert bool((c.ev[pad] == 0).all())
        # padding rows inside and at the end of a polarity block (blocks of a single row have none)
        blocks = [(0, c.num_pos), (c.num_pos, c.M)] if c.split else [(0, c.M)]
        for lo, hi in blocks:
            if hi - lo > 4 and not name.startswith('polarity'):
                assert bool(pad[:, hi - 1].all()), (name, 'no padding at the end of a block')
                live_after_pad = [bool(pad[b, lo:i].any()) for b in range(c.B) for i in range(lo, hi) if not pad[b, i]]
                assert any(live_after_pad), (name, 'no padding inside a block')


def test_cases_are_deterministic():
    for name in ('rows_and_columns', 'weights', 'polarity_npM1'):
        fn, args = E.CASES[name]
        a, b = fn(name, *args), E.case(name)
        for key in ('ev', 'lut', 'gimg', 'add', 'kind'):
            assert np.array_equal(getattr(a, key), getattr(b, key)), (name, key)


def test_edges_are_where_the_names_say():
    d = lambda name: (E.case(name), E.decisions(E.case(name)))        # noqa: E731
    c, dd = d('rows_and_columns')
    y, x, live = dd['y'][..., 0], dd['x'][..., 0], dd['live'][..., 0]
    for r in range(-1, c.H + 1):
        assert int((dd['y0f'][..., 0] == r).sum()) >= 4, r                # every row is a top tap row ...
    for q in range(-1, c.W + 1):
        assert int((dd['x0f'][..., 0] == q).sum()) >= 4, q
    assert int(((y == 0) & live).sum()) > 0 and int(((y == c.H) & live).sum()) > 0 and int(((x == c.W) & live).sum()) > 0
    assert int(((y < 0) & ~live & (c.kind > 0)).sum()) > 0                   # ... and the mask drops what lies outside
    frac = y - dd['y0f'][..., 0]
    assert int(((frac == np.float32(2.0 ** -20)) & live).sum()) >= c.H
    # one-row strips: the first workgroup of k_ev_bin has more records than it can stage (two forward, one backward per live row)
    inside = live & dd['near'][..., 0]
    assert 3 * int(inside[0, :E.EV_CHUNK].sum()) > E.EV_STAGE
    c, dd = d('rows_and_columns_nomask')
    assert int(((dd['y0f'][..., 0] == -1) & dd['live'][..., 0]).sum()) > 0 and int(((dd['x0f'][..., 0] == -1) & dd['live'][..., 0]).sum()) > 0
    c, dd = d('below_integer')
    fy, fx = dd['y'] - dd['y0f'], dd['x'] - dd['x0f']
    assert int(((fy < 0) & dd['live']).sum()) >= c.H // 2 and int(((fx < 0) & dd['live']).sum()) >= c.W // 2
    c, dd = d('weights')
    w = dd['w'][..., 0]
    for v in (1e-6, 1.5, np.nextafter(np.float32(1.5), np.float32(2)), 1.9999, 2.5, -2.5, 1000.0, -1000.0):
        assert int((w == np.float32(v)).sum()) > 0, v
    kinds = np.array(c.kinds)[c.kind]
    assert bool((w[(kinds == 'dt>=1') | (kinds == 'dt=1.3') | (kinds == 'dt=-1.3')] == 0).all())
    assert bool(((np.abs(w[kinds == 'dt~1']) > 0) & (np.abs(w[kinds == 'dt~1']) < 3e-6)).all())
    for name in ('polarity_np1', 'polarity_npM1', 'polarity_mid_last_sample'):
        c, dd = d(name)
        rows = [b for b in range(c.B) if dd['live'][b, c.num_pos - 1, 0] and dd['live'][b, c.num_pos, 0]]
        assert rows, name
    for name in ('polarity_mid_last_sample', 'polarity_off_last_sample'):
        c, dd = d(name)
        assert not dd['live'][:-1].any() and dd['live'][-1].any()
    assert [E.case(n).num_pos for n in ('polarity_np0', 'polarity_np1')] == [0, 1]
    assert E.case('polarity_npM1').num_pos == E.case('polarity_npM1').M - 1 and E.case('polarity_npM').num_pos == E.case('polarity_npM').M
    c, dd = d('clamped_cells')
    kinds = np.array(c.kinds)[c.kind]
    for k in ('y<0', 'y>=H', 'x<0', 'x>=W', 'bin<0', 'bin>=nb'):
        assert int((dd['live'][..., 0] & dd['near'][..., 0] & (kinds == k)).sum()) > 20, k      # they come back inside
    for name in ('far_flows', 'far_flows_masked'):
        c, dd = d(name)
        far = np.char.startswith(np.array(c.kinds)[c.kind], 'far')
        assert int(far.sum()) > 100 and not (dd['near'][..., 0] & dd['live'][..., 0] & far).any()
    for name in ('lut_seams', 'lut_seams_tall'):
        c = E.case(name)
        iy = E.cell_of(c.ev[..., 0], 1, c.H)[c.kind > 0]
        assert set(iy.tolist()) == set(range(c.H))
        n = E.expected_bwd(name, True)['n']
        assert int((n[:, 1, 16:] > 0).sum()) == 0 and int((n[:, 1, :8] > 0).sum()) > 0
    c = E.case('tiny_strip')
    n = E.expected_bwd('tiny_strip', False)['n']
    assert int((n.reshape(c.B, c.nb, -1, 2)[..., 0] > 0).sum(-1).max()) == 1 and int(n.max()) > 300
    c = E.case('large_adjoint')
    assert float(np.abs(c.gimg).max()) == 1e4 and float(np.abs(c.ev[..., 5]).max()) == 50.0
    assert float(np.abs(E.expected_bwd('large_adjoint', False)['ref']).max()) < 2.0 ** 30 * abs(E.GCOEF * E.GOUT)


def test_comparator_rejects_what_it_should():
    ref, allow = np.array([[1.0, 0.0], [2.0, 0.0]]), np.array([[1e-6, 0.0], [1e-6, 0.0]])
    assert E.compare(ref, ref, allow).ratio == 0.0
    r = E.compare(ref + np.array([[0.0, 0.0], [5e-7, 0.0]]), ref, allow)
    assert abs(r.ratio - 0.5) < 1e-6 and r.index == (1, 0)
    assert E.compare(ref + np.array([[0.0, 1e-30], [0.0, 0.0]]), ref, allow) == E.Result(float('inf'), (0, 1), ())
    assert E.compare(ref + np.array([[np.nan, 0.0], [0.0, 0.0]]), ref, allow).ratio == float('inf')
    with pytest.raises(AssertionError):
        E.check('x', 'y', ref + 2e-6, ref, allow)
