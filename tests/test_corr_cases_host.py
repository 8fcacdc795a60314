"""The correlation-lookup cases of tests/corr_cases.py on the CPU: the float64 reference against the five g16_corr fixtures and,
away from integers, against float64 autograd through the plain-torch mirror; the centre replay against its own bound; what the
named cases claim to reach, asserted from the case data; and the comparator itself -- a float32 restatement of the kernels'
expressions passes it on every case, and nine mutants of it fail with an assertion that names the first bad element."""
import re

import pytest
import torch

import corr_cases as CK
from conftest import load_golden


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _fixture_case(g):
    from motionpriorcmax_amd import utils
    nl = [int(v) for v in g['num_levels']]
    levels, tix = utils.corr_pyramid(torch.from_numpy(g['fmap1']), torch.from_numpy(g['fmap2']), nl)
    params, times = torch.from_numpy(g['params']), [float(t) for t in g['times']]
    d = params.shape[1] // 2
    cs = CK._case('fixture', params.shape[0], params.shape[2], params.shape[3], nl, int(g['radius']), d, 0, params=params)
    cs.levels, cs.g, cs.times, cs.basis = [lv.detach() for lv in levels], torch.from_numpy(g['g']), times, CK.basis_of(times, d)
    assert cs.tix == tix
    return cs


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e'])
def test_reference_equals_the_fixtures_float64(name):
    """The fixtures' float64 tensors keep 29 significant bits (tools/gen_golden_corr.py: keep29), so agreement is 2^-28 relative per
    element, plus 2^-45 of the tensor's maximum for the order of the float64 sums."""
    g = load_golden('g16_corr_' + name)
    cs = _fixture_case(g)
    ref = CK.reference(cs, centres=CK.centres64(cs.params, cs.basis))
    pairs = [('out', ref.out), ('grad_coords', ref.gc), ('grad_params', ref.gp)] + [(f'grad_level_{l}', t) for l, t in enumerate(ref.gl)]
    for key, got in pairs:
        want = torch.from_numpy(g[key + '64'])
        err = (got.reshape(want.shape) - want).abs()
        tol = 2.0 ** -28 * want.abs() + 2.0 ** -45 * float(want.abs().max())
        print(f'{name} {key}: max |reference - fixture| {float(err.max()):.3e} (max {float(want.abs().max()):.3e})')
        assert bool((err <= tol).all()), (name, key, float(err.max()))


MIRROR_MARGIN = 2.0 ** -14


def _margin(cs):
    c = cs.coords.double()
    return min(float((c * 0.5 ** l - torch.round(c * 0.5 ** l)).abs().min()) for l in range(len(cs.levels)))


@pytest.mark.parametrize('name', ['r1', 'r2', 'r3', 'r4', 'd1', 'offset_views'])
def test_reference_equals_the_mirror_away_from_integers(name):
    """float64 autograd through utils.corr._lookup_mirror at the same fp32 centres.  The mirror maps x to 2 x / (W - 1) - 1 and
    grid_sample maps back: a few float64 roundings of numbers up to |x| + W, 2^-48 (|x| + W) at the very most -- far inside the
    case's distance from an integer, so both take the same cell, and the outputs differ by that times the slope."""
    from motionpriorcmax_amd.utils.corr import _lookup_mirror
    cs = CK.case(name)
    assert _margin(cs) >= MIRROR_MARGIN, _margin(cs)
    ref = CK.expected(name)
    c = cs.coords.double().requires_grad_(True)
    lv = [t.double().requires_grad_(True) for t in cs.levels]
    out = _lookup_mirror(lv, cs.tix, cs.r, c)
    grads = torch.autograd.grad(out, [c] + lv, cs.g.double())
    delta = 2.0 ** -48 * (float(cs.coords.abs().max()) + cs.w)
    vmax, gmax, K2 = max(float(t.abs().max()) for t in cs.levels), float(cs.g.abs().max()), (2 * cs.r + 1) ** 2
    assert float((out.detach() - ref.out).abs().max()) <= 2 * vmax * delta + 2.0 ** -50 * vmax
    # the coordinate gradient is piecewise constant in the own axis and linear in the other: slope 4 max |V| per output
    assert float((grads[0] - ref.gc).abs().max()) <= len(cs.levels) * K2 * gmax * (4 * vmax * delta + 2.0 ** -48 * vmax)
    for a, b in zip(grads[1:], ref.gl):
        assert float((a - b).abs().max()) <= 4 * gmax * (delta + 2.0 ** -50)


@pytest.mark.parametrize('name', CK.BEZIER_CASES)
def test_replayed_centres_lie_within_their_bound_of_the_float64_centres(name):
    cs = CK.case(name)
    c64, bound = CK.centres64(cs.params, cs.basis), CK.replay_bound(cs.params, cs.basis)
    fin = torch.isfinite(c64) & torch.isfinite(cs.coords.double())
    assert cs.coords.dtype == torch.float32 and torch.equal(cs.coords.view(torch.int32), CK.replay_centres(cs.params, cs.basis).view(torch.int32))
    err = (cs.coords.double() - c64).abs()
    assert bool((err[fin] <= bound[fin]).all())
    pos = fin & (bound > 0)
    print(f'{name}: replayed centre against float64, largest ratio {float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0:.3f}')
    if name != 'nonfinite_bezier':
        assert bool(fin.all())


# ---- what the cases reach -------------------------------------------------------------------------------------------------------
def test_every_level_is_at_least_2_by_2_and_the_descriptor_is_served():
    import ctypes
    from motionpriorcmax_amd import _lib as C
    from test_corr_lookup_host import descriptor
    for name in CK.CASES:
        cs = CK.case(name)
        assert all(min(lv.shape[-2:]) >= 2 for lv in cs.levels)
        assert C.lib().mpc_corr_lookup_supported(ctypes.byref(descriptor(cs.h, cs.w, cs.nl, cs.r, cs.d, cs.B))) == 0, name
    assert set(CK.BEZIER_CASES) | {'lattice', 'neg_fraction', 'nonfinite'} == set(CK.CASES)


def test_zero_params_samples_at_integers_halves_and_quarters():
    cs = CK.case('zero_params')
    assert not bool(cs.params.any()) and len(cs.levels) == 3
    assert torch.equal(cs.coords, CK._grid(cs.T, cs.B, cs.h, cs.w))
    for l, want in enumerate(({0.0}, {0.0, 0.5}, {0.0, 0.25, 0.5, 0.75})):
        assert set(CK.fractions32(cs, l).reshape(-1).tolist()) == want


def test_lattice_reaches_every_clipping_state():
    cs = CK.case('lattice')
    r = cs.r
    x0, y0 = CK.scaled_cells(cs, 0)
    # from the window one column left of the slice (x0 = -r - 2) to the one past its right edge: every state between, and in
    # particular the window that touches column 0 only (x0 = -r - 1) and the one that touches the last column only (w - 1 + r)
    assert set(x0.reshape(-1).tolist()) == set(range(-r - 2, cs.w + r + 2))
    assert set(y0.reshape(-1).tolist()) == set(range(-r - 2, cs.h + r + 2))
    assert -r - 1 in x0 and cs.w - 1 + r in x0 and -r - 1 in y0 and cs.h - 1 + r in y0
    fr = CK.fractions32(cs, 0)
    for axis in (0, 1):
        cells = (x0, y0)[axis]
        for v in range(-r - 2, (cs.w, cs.h)[axis] + r + 2):
            assert set(fr[:, :, axis][cells == v].tolist()) == {0.0, 0.25, 0.5, 0.75}, (axis, v)
    assert set(CK.fractions32(cs, 1).reshape(-1).tolist()) == {k / 8 for k in range(8)}


def test_neg_fraction_holds_both_intervals_and_a_fraction_of_one():
    cs = CK.case('neg_fraction')
    for l in range(2):
        s = cs.coords.double() * 0.5 ** l
        fr = CK.fractions32(cs, l)
        for axis in (0, 1):
            sa, fa = s[:, :, axis], fr[:, :, axis]
            assert bool(((sa > -0.5) & (sa < 0)).any()) and bool(((sa > -1) & (sa < -0.5)).any())
            assert bool((fa == 1.0).any()), 'fx == 1.0f does not occur'
            inexact = fa.double() != sa - torch.floor(sa)
            assert bool(inexact.any()) and bool(((sa > -0.5) & (sa < 0))[inexact].all())        # only that interval is inexact
            assert float((fa.double() - (sa - torch.floor(sa))).abs().max()) <= CK.U / 2
    assert -2.0 ** -30 in cs.coords[0, 0, 0] and -2.0 ** -30 in cs.coords[0, 0, 1]


def test_radius_cases_reach_the_chunk_tails_and_both_store_paths():
    hw = {name: CK.case(name).h * CK.case(name).w for name in ('r1', 'r2', 'r3', 'r4')}
    assert hw == dict(r1=63, r2=64, r3=65, r4=130) and [CK.case(f'r{r}').r for r in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert hw['r1'] % CK.CHUNK == 63 and hw['r2'] % CK.CHUNK == 0 and hw['r3'] % CK.CHUNK == 1 and hw['r4'] // CK.CHUNK == 2
    cs = CK.case('r4')
    assert cs.B == 3 and (cs.B * cs.h * cs.w) % 4 != 0
    widths = {lv.shape[-1] for name in ('r1', 'r2', 'r3', 'r4') for lv in CK.case(name).levels}       # every level receives a gradient
    assert any(v % 4 == 0 for v in widths) and any(v % 4 for v in widths)
    for name in ('r1', 'r2'):                                                    # per case: both store paths of the slice fill
        ws = [lv.shape[-1] for lv in CK.case(name).levels]
        assert any(v % 4 == 0 for v in ws) and (name == 'r2' or any(v % 4 for v in ws))
    assert (2 * 3 + 2) ** 2 == CK.CHUNK                                           # radius 3: the window fills one pass of a wave


def test_limit_cases_reach_the_limits():
    from motionpriorcmax_amd import _lib as C
    cs = CK.case('limits_targets')
    assert cs.T == C.CORR_MAX_TARGETS == 16 and cs.d == 16 and (cs.h, cs.w) == (8, 9) and len(cs.levels) == 3
    for l in (1, 2):                                                             # (level 0 holds every target: the identity)
        assert cs.tix[l] != list(range(len(cs.tix[l]))) and all(t != k for k, t in enumerate(cs.tix[l]))
    full = CK.case('limits_full')
    assert full.T == 16 and full.d == 16 and full.E == 48 and all(len(t) == 16 for t in full.tix)
    assert CK.case('d1').d == 1 and CK.case('d1').r == C.CORR_MAX_RADIUS == 4
    six = CK.case('six_levels')
    assert len(six.levels) == C.CORR_MAX_LEVELS == 6 and tuple(six.levels[5].shape[-2:]) == (2, 2) and six.r == 1
    assert six.levels[0].numel() * 4 == 64 << 20
    assert max(CK.case(n).levels[0].numel() for n in CK.CASES if n != 'six_levels') * 4 < 4 << 20


@pytest.mark.parametrize('name', ['nonfinite', 'nonfinite_bezier'])
def test_nonfinite_cases_give_zero_where_they_should(name):
    cs, ref = CK.case(name), CK.expected(name)
    src = cs.coords if name == 'nonfinite' else cs.params
    for v in CK.NONFINITE:
        assert bool(torch.isnan(src).any()) if v != v else bool((src == v).any()), v
    c = cs.coords.double()
    badc = (~torch.isfinite(c) | (c.abs() >= 2.0 ** 20)).any(dim=2)               # [T, B, h, w]
    assert int(badc.sum()) >= len(CK.NONFINITE)
    K2 = (2 * cs.r + 1) ** 2
    e = 0
    for l, ts in enumerate(cs.tix):
        for k, t in enumerate(ts):
            o = ref.out[:, e * K2:(e + 1) * K2].permute(0, 2, 3, 1)[badc[t]]
            assert o.numel() and not bool(o.any()) and not bool(ref.e_out[:, e * K2:(e + 1) * K2].permute(0, 2, 3, 1)[badc[t]].any())
            sl = ref.gl[l][k].reshape(cs.B, cs.h, cs.w, -1)[badc[t]]
            assert not bool(sl.any()) and not bool(ref.e_gl[l][k].reshape(cs.B, cs.h, cs.w, -1)[badc[t]].any())
            e += 1
    gcb = ref.gc.permute(0, 1, 3, 4, 2)[badc]
    assert not bool(gcb.any()) and not bool(ref.e_gc.permute(0, 1, 3, 4, 2)[badc].any())
    pix = badc.any(0)[0].reshape(-1)
    assert bool(pix[:CK.CHUNK].any()) and bool(pix[CK.CHUNK:].any()) and int(pix.sum()) < 16        # scattered over both chunks
    for t in [ref.out, ref.gc] + ref.gl + ([ref.gp] if cs.params is not None else []):
        assert bool(torch.isfinite(t).all())
    assert float(ref.out.abs().max()) > 0 and float(ref.gc.abs().max()) > 0


def test_offset_views_is_marked_and_has_a_level_that_would_take_the_wide_store():
    cs = CK.case('offset_views')
    assert cs.offset and any(lv.shape[-1] % 4 == 0 for lv in cs.levels) and [n for n in CK.CASES if CK.case(n).offset] == ['offset_views']


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def _check(name, mutant=None, accum=False):
    cs = CK.case(name)
    ref = CK.expected(name)
    label = name if mutant is None else f'{name} [{mutant}]'
    worst = 0.0
    if accum:
        pf = CK.prefill(cs)
        return CK.compare_accum(label, ref, pf, CK.f32_lookup(cs, mutant=mutant, prefill=pf).gl)
    got = CK.f32_lookup(cs, mutant=mutant)
    worst = CK.compare_all(label + ' coords', ref, out=got.out, gc=got.gc, gl=got.gl)
    if cs.params is not None:
        gb = CK.f32_lookup(cs, bezier=True, mutant=mutant)
        assert torch.equal(gb.out, got.out) or mutant is not None
        worst = max(worst, CK.compare_all(label + ' bezier', ref, out=gb.out, gp=gb.gp))
    return worst


@pytest.mark.parametrize('name', CK.CASES)
def test_float32_restatement_passes(name):
    worst = _check(name)
    assert worst < 1.0
    assert _check(name, accum=True) < 1.0


# (mutant, the named case that must catch it, the output that names the first bad element)
CAUGHT = [('trunc', 'lattice', 'out'), ('trunc', 'neg_fraction', 'out'), ('round', 'r1', 'out'), ('round', 'zero_params', 'out'),
          ('edge_clamp', 'lattice', 'out'), ('edge_clamp', 'r4', 'out'), ('swap_w01_w10', 'r1', 'out'), ('swap_w01_w10', 'r3', 'out'),
          ('origin', 'r2', 'out'), ('origin', 'zero_params', 'out'), ('no_level_scale', 'r1', 'grad_coords'),
          ('no_level_scale', 'zero_params', 'grad_coords'), ('target_major', 'r4', 'out'), ('target_major', 'limits_targets', 'out'),
          ('slot_as_target', 'limits_targets', 'out'), ('unwritten_cell', 'r2', 'grad_level_fill'),
          ('unwritten_cell', 'offset_views', 'grad_level_fill')]


def test_every_named_mutant_is_listed():
    assert {m for m, _, _ in CAUGHT} == set(CK.MUTANTS) and len(CK.MUTANTS) == 9


@pytest.mark.parametrize('mutant,name,where', CAUGHT)
def test_mutants_fail_the_comparator(mutant, name, where):
    """floor replaced by trunc / by round, clamp-to-edge for zero per tap, w01 and w10 swapped, the window origin off by one, the
    2^-l missing from the coordinate gradient, entries target-major, slot k of a level above 0 read as target k, one in-window
    grad_level cell left unwritten: each is caught on a named case, by the output it corrupts first."""
    with pytest.raises(AssertionError, match='first bad element') as e:
        _check(name, mutant)
    assert re.search(rf'\] (coords|bezier)( level \d)? {where}: first bad element \(', str(e.value)), str(e.value)


def test_a_mutant_corrupts_the_elements_it_should():
    """trunc differs from floor only at negative non-integer coordinates; the unwritten cell is one element."""
    cs, ref = CK.case('lattice'), CK.expected('lattice')
    got = CK.f32_lookup(cs, mutant='trunc')
    bad = ~((got.out.double() - ref.out).abs() <= ref.e_out)
    K2 = (2 * cs.r + 1) ** 2
    e = 0
    for l, ts in enumerate(cs.tix):
        s = cs.coords.double() * 0.5 ** l
        neg = ((s < 0) & (s != torch.floor(s))).any(dim=2)                        # [T, B, h, w]
        for t in ts:
            assert not bool(bad[:, e * K2:(e + 1) * K2].permute(0, 2, 3, 1)[~neg[t]].any())
            e += 1
    assert bool(bad.any())
    got = CK.f32_lookup(CK.case('r2'), mutant='unwritten_cell')
    r2 = CK.expected('r2')
    assert sum(int((~((t.double() - a).abs() <= b)).sum()) for t, a, b in zip(got.gl, r2.gl, r2.e_gl)) == 1
