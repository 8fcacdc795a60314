"""FocusLoss.calc_per_event_curves(curve_type='BSPLINE'), host side: the fp32 mirror utils.curve_event_basis(..., 'BSPLINE') -- the
DEFINITION the kernels restate -- against a scalar restatement of its lines, against float64 Cox-de Boor within a derived bound, its
exact end points, its support of four, its reduction to the cubic Bezier curve at d = 3; the d < 3 rule, the routing, and the LUT
route's name for the same curve (utils.curve_basis('BSPLINE')).  (GPU side: tests/test_gpu_pe_bspline.py.)"""
import numpy as np
import pytest
import torch

import pe_bspline_cases as BC
import pe_curves_cases as PC
from oracle import focus_oracle as O

DEGREES = [3, 4, 5, 7, 10, 16]


def _times(d, dense=20001):
    """A dense grid, 0, 1, every knot with its fp32 neighbours, and times slightly outside [0, 1] (clamped)."""
    outside = torch.tensor([-1e-3, -2.0 ** -30, 1.0 + 2.0 ** -23, 1.5, -7.0])
    g = torch.Generator().manual_seed(d)
    return torch.cat((BC.knot_times(d), outside, torch.linspace(0, 1, dense), torch.rand(dense, generator=g)))


def _scalar_lines(t, d):
    """The definition's lines for one time, one np.float32 operation each."""
    f = np.float32
    L = d - 2
    tc = min(max(f(t), f(0)), f(1))
    x = f(tc * f(L))
    s = min(int(np.floor(x)), L - 1)
    u = {k: f(min(max(s + k, 0), L)) for k in range(-2, 4)}
    N = [f(1), f(0), f(0), f(0)]
    for j in range(1, 4):
        saved = f(0)
        for r in range(j):
            right, left, den = f(u[r + 1] - x), f(x - u[1 - j + r]), f(u[r + 1] - u[1 - j + r])
            assert den in (1, 2, 3)
            temp = f(N[r] / den)
            N[r] = f(saved + f(right * temp))
            saved = f(left * temp)
        N[j] = saved
    E = np.zeros(d + 1, dtype=np.float32)
    for q in range(4):
        E[s + q] = N[q]
    return E[1:], s


@pytest.mark.parametrize('d', DEGREES)
def test_mirror_is_the_definitions_lines_bit_for_bit(d):
    """(a), mirror side: the vectorised torch lines equal the scalar ones at every knot, its neighbours, outside [0, 1] and on a
    coarse grid."""
    from motionpriorcmax_amd.utils import curve_event_basis
    t = torch.cat((_times(d, dense=0), torch.linspace(0, 1, 301)))
    got = curve_event_basis(t, d, 'BSPLINE')
    assert got.dtype == torch.float32 and tuple(got.shape) == (t.numel(), d)
    want = np.stack([_scalar_lines(float(v), d)[0] for v in t])
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('d', DEGREES)
def test_mirror_against_float64_cox_de_boor(d):
    """(b) exact end points, (c) at most four non-zeros, all inside [s - 1, s + 2], (d) every element within the derived bound of the
    float64 recursion (pe_bspline_cases.basis_bound: 3 ulp(x) / 2 + 12 roundings).  Measured: 8.9e-8 (d = 3), 1.1e-7 (d = 4, 10),
    7.3e-7 (d = 7), 1.4e-6 (d = 16)."""
    from motionpriorcmax_amd.utils import curve_event_basis
    t = _times(d)
    L = d - 2
    got = curve_event_basis(t, d, 'BSPLINE')
    want = BC.bspline64(t, d)
    x = t.clamp(0, 1) * float(L)                          # the definition's x, fp32
    bound = BC.basis_bound(x)[:, None]
    err = (got.double() - want).abs()
    print(f'd={d}: worst |E_fp32 - E_float64| {float(err.max()):.3e}, bound there {float(bound.expand_as(err)[err == err.max()][0]):.3e}, '
          f'largest bound {float(bound.max()):.3e}')
    assert (err <= bound).all(), float((err - bound).max())
    # (b) t = 0 (and anything clamped to it): exactly zero; t = 1 (and beyond): exactly one-hot on E_d
    last = (torch.arange(d) == d - 1).float()
    for v, row in ((0.0, torch.zeros(d)), (-7.0, torch.zeros(d)), (1.0, last), (1.5, last)):
        e = curve_event_basis(torch.tensor([v]), d, 'BSPLINE')[0]
        assert torch.equal(e, row) and not torch.signbit(e).any(), (v, e)
    # (c) the support: E index j (0-based) non-zero only for s - 1 <= j <= s + 2
    s = x.floor().long().clamp(max=L - 1)
    j = torch.arange(d)[None, :]
    outside = (j < s[:, None] - 1) | (j > s[:, None] + 2)
    assert int((got != 0).sum(-1).max()) <= 4
    assert float(got[outside].abs().max() if outside.any() else 0.0) == 0.0 and not torch.signbit(got[outside]).any()
    # a partition of unity with the dropped N_0, to the same bound
    n0 = 1.0 - want.sum(-1)
    assert ((got.double().sum(-1) + n0 - 1.0).abs() <= 4 * bound[:, 0]).all()


def test_degree_5_picks_the_span_from_the_rounded_x():
    """d = 5: the knots 1/3 and 2/3 are not fp32 numbers; x = fl(t * 3) decides the span.  fl(1/3) * 3 rounds to exactly 1.0 (span 1),
    its lower neighbour stays below (span 0) -- and the values agree across the knot to the bound either way."""
    from motionpriorcmax_amd.utils import curve_event_basis
    t13 = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    dn = torch.nextafter(t13, torch.tensor(0.0))
    assert float(t13 * 3.0) == 1.0 and float(dn * 3.0) < 1.0
    assert _scalar_lines(float(t13), 5)[1] == 1 and _scalar_lines(float(dn), 5)[1] == 0
    e = curve_event_basis(torch.stack((dn, t13)), 5, 'BSPLINE')
    assert float(e[1, 3]) == 0.0 and float(e[0, 3]) == 0.0          # N_4 starts at the knot with a triple zero
    assert (e[0] - e[1]).abs().max() <= 2 * BC.basis_bound_of_degree(5)


def test_degree_3_is_the_cubic_bezier_curve():
    """(e): one span, the Bernstein polynomials -- within 6e-8 measured; held to the two kinds' own bounds against float64 (BEZIER:
    2d roundings relative, tests/test_pe_curves_host.py)."""
    from motionpriorcmax_amd.utils import curve_event_basis
    t = _times(3)
    a, b = curve_event_basis(t, 3, 'BSPLINE'), curve_event_basis(t.clamp(0, 1), 3, 'BEZIER')
    worst = float((a - b).abs().max())
    print(f'BSPLINE d=3 against BEZIER d=3: {worst:.3e}')
    assert worst <= BC.basis_bound_of_degree(3) + 6 * 2.0 ** -24
    t64 = t.clamp(0, 1).double()
    want = torch.stack((3 * (1 - t64) ** 2 * t64, 3 * (1 - t64) * t64 ** 2, t64 ** 3), dim=-1)          # the Bernstein polynomials, float64
    assert (BC.bspline64(t, 3) - want).abs().max() <= 1e-15


def test_float64_recursion_against_scipy():
    """The tests' own Cox-de Boor pinned to scipy.interpolate.BSpline (host test only)."""
    si = pytest.importorskip('scipy.interpolate')
    for d in DEGREES:
        L = d - 2
        knots = np.concatenate((np.zeros(3), np.arange(L + 1) / L, np.ones(3)))
        t = _times(d, dense=2001).clamp(0, 1).double()
        want = np.stack([si.BSpline(knots, np.eye(d + 1)[i], 3)(t.numpy()) for i in range(1, d + 1)], axis=-1)
        assert np.abs(BC.bspline64(t, d).numpy() - want).max() <= 1e-14


def _loss(**over):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', PC.loss_cfg(**over))


def test_fewer_than_three_control_points_raise_a_value_error_that_names_the_rule():
    from motionpriorcmax_amd.utils import curve_event_basis, curve_basis
    L = _loss()
    ev, num_pos = O.synth_events(2, 100, PC.SHAPE, PC.NB, seed=1)
    batch = {'events': ev, 'num_pos_events': num_pos}
    for d in (1, 2):
        with pytest.raises(ValueError, match='d >= 3'):
            L.calc_per_event_curves(torch.zeros(2, 2 * d, PC.HQ, PC.WQ), 0.4, batch, curve_type='BSPLINE')
        with pytest.raises(ValueError, match='d >= 3'):
            curve_event_basis(torch.zeros(3), d, 'BSPLINE')
        with pytest.raises(ValueError, match='degree >= 3'):
            curve_basis('BSPLINE', [0.0, 0.5], d)
    with pytest.raises(ValueError, match='go together'):
        L.calc_per_event_curves(torch.zeros(2, 6, PC.HQ, PC.WQ), 0.4, batch, curve_type='BSPLINE', basis_table=torch.zeros(9, 3))
    with pytest.raises(ValueError, match='go together'):
        curve_event_basis(torch.zeros(3), 3, 'BSPLINE', torch.zeros(9, 3))
    from motionpriorcmax_amd import ops
    assert ops.PEC_BASIS['BSPLINE'] == 3
    assert ops.pec_supported(L._cfg, ev, num_pos, 10, 'BSPLINE') == 0          # (CPU events: the library is not asked)


def test_routing(monkeypatch):
    """'BSPLINE' runs ops.PerEventCurvesFn with no table where the library serves it; fused=False and what mpc_pec_supported
    refuses (d > 16) take the existing per-event nodes with phi [B, M, d] from the mirror."""
    from motionpriorcmax_amd import ops
    from motionpriorcmax_amd.utils import curve_event_basis
    L = _loss(smooth_weight=0.0)
    ev, num_pos = O.synth_events(2, 50, PC.SHAPE, PC.NB, seed=1)
    batch = {'events': ev, 'num_pos_events': num_pos}
    seen = []

    class Fused:
        @staticmethod
        def apply(params, up_mask, events, t_ref, phim, cfg, num_pos, offsets, curve_type, table, scale, tile):
            seen.append(('fused', curve_type, table, tile, params.shape[1] // 2))
            z = torch.zeros(())
            return z, z, z, torch.zeros(2, 2, *PC.SHAPE)

    class Unfused:
        @staticmethod
        def apply(c_rows, events, phi, t_ref, cfg, num_pos, offsets=None):
            seen.append(('unfused', tuple(c_rows.shape), phi))
            return torch.zeros(()), torch.zeros(2, 2, *PC.SHAPE)

    asked = []

    def supported(cfg, events, num_pos, d, curve_type, samples=0):
        asked.append((d, curve_type, samples))
        return 0 if d > 16 else 3

    monkeypatch.setattr(ops, 'PerEventCurvesFn', Fused)
    monkeypatch.setattr(ops, 'PerEventBasisFocusFn', Unfused)
    monkeypatch.setattr(ops, 'pec_supported', supported)
    G = PC.HQ * PC.WQ
    L.calc_per_event_curves(torch.zeros(2, 20, PC.HQ, PC.WQ), 0.4, batch, curve_type='BSPLINE')
    assert seen[-1] == ('fused', 'BSPLINE', None, 4, 10) and asked[-1] == (10, 'BSPLINE', 0)
    L.calc_per_event_curves(torch.zeros(2, 20, PC.HQ, PC.WQ), 0.4, batch, curve_type='BSPLINE', fused=False)
    assert seen[-1][:2] == ('unfused', (2 * G, 20))
    tr = torch.full((1,), 0.4)
    assert torch.equal(seen[-1][2], curve_event_basis(tr, 10, 'BSPLINE') - curve_event_basis(ev[..., 2], 10, 'BSPLINE'))
    L.calc_per_event_curves(torch.zeros(2, 34, PC.HQ, PC.WQ), 0.4, batch, curve_type='BSPLINE')                     # d = 17
    assert seen[-1][:2] == ('unfused', (2 * G, 34)) and tuple(seen[-1][2].shape) == (2, 50, 17) and asked[-1] == (17, 'BSPLINE', 0)


def test_the_lut_route_names_the_same_curve():
    """utils.curve_basis('BSPLINE') is the bspline_basis matrix and trajectories_from_curves(curve_type='BSPLINE') gives the bits of
    trajectories_from_bspline, with and without the convex-upsampling mask."""
    from motionpriorcmax_amd import utils
    times = torch.cat((torch.tensor([0.41]), O.bin_mid_times(PC.NB)))
    for d in (3, 7, 10):
        bm = utils.curve_basis('BSPLINE', times, d)
        assert bm.dtype == torch.float32 and torch.equal(bm, utils.bspline_basis(times, d + 1))
        assert torch.equal(utils.curve_basis('BSPLINE', times, d, scalar_time_shortcuts=True), bm)
        # ... and it is the curve the per-event kind evaluates, to that kind's bound
        assert (bm.double() - utils.curve_event_basis(times, d, 'BSPLINE').double()).abs().max() <= BC.basis_bound_of_degree(d) + 2.0 ** -24
    g = torch.Generator().manual_seed(5)
    d = 7
    p = torch.randn(2, 2 * d, PC.HQ, PC.WQ, generator=g)
    a, pa = utils.trajectories_from_curves(p, times, PC.SP, PC.SHAPE, curve_type='BSPLINE', scale=1.5)
    b, pb = utils.trajectories_from_bspline(p, times, PC.SP, PC.SHAPE, scale=1.5)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    p8, m8 = torch.randn(2, 2 * d, 12, 16, generator=g), torch.randn(2, 576, 12, 16, generator=g)
    a, _ = utils.trajectories_from_curves(p8, times, PC.SP, PC.SHAPE, curve_type='BSPLINE', up_mask=m8)
    b, _ = utils.trajectories_from_bspline(p8, times, PC.SP, PC.SHAPE, up_mask=m8)
    assert torch.equal(a, b)
    f = utils.flows_from_curves(p8, times, curve_type='BSPLINE', up_mask=m8)
    assert tuple(f.shape) == (times.numel(), 2, 2, *PC.SHAPE) and float(f[0].abs().max()) > 0


@pytest.mark.parametrize('name', list(BC.CASES))
def test_the_accounting_excuses_a_minority_of_the_tiles(name):
    """From the definition's positions alone, before anything runs on a GPU: the explained share of every case is below the 25 %
    cap of assert_accountable -- and an fp32 restatement of the definition (the mirror as E) meets the caps."""
    from motionpriorcmax_amd.utils import curve_event_basis
    cfg, ev, num_pos, *_ = BC.case_inputs(name)
    ref = BC.reference(name)
    tiles, _ = PC.explained_tiles(cfg, ev, num_pos, ref['warped'], ref['iwes'])
    share = float(tiles.float().mean())
    print(f'{name}: explained share {100 * share:.2f} %')
    assert share < 0.25
    assert np.isfinite(ref['loss']) and float(ref['g_rows'].abs().max()) > 0
    w = ref['warped'][:, 0]
    out = ((w[..., 0] < 0) | (w[..., 0] > PC.SHAPE[0]) | (w[..., 1] < 0) | (w[..., 1] > PC.SHAPE[1])).float().mean()
    assert 0 < float(out) < 0.5
    d = BC.CASES[name]['d']
    r32 = BC.define(name, basis=lambda t: curve_event_basis(t.float(), d, 'BSPLINE'), dtype=torch.float32)
    res = BC.rows_accounting(name, r32['g_rows'], label=name + ' (fp32 restatement)')
    print(f'{name}: fp32 restatement: {res}')
    assert abs(r32['loss'] - ref['loss']) <= 1e-5 * abs(ref['loss'])
