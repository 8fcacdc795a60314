"""The correlation-pyramid cases of tests/corr_pyramid_cases.py on the CPU: the exactness precondition of every case, the Python
restatement of the plan against the library's workspace sizes, what the named cases claim to reach (a census taken while the tiling
is walked, asserted per product), and the comparator itself -- a float64 restatement of the kernels' tiling passes it on every
case, and six mutants of it fail with an assertion that names the first bad element, on exactly the cases listed."""
import ctypes
import re

import pytest
import torch

import corr_pyramid_cases as PK


def _desc(cs):
    from motionpriorcmax_amd import ops
    desc, tix = ops.corr_pyramid_desc(cs.B, cs.h, cs.w, cs.nl)
    assert tix == cs.tix
    return desc


# ---- preconditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PK.CASES)
def test_every_sum_is_exact_and_the_reference_representable(name):
    """expected() asserts A * sqrt(D) * 4^(L-1) < 2^24 for every output and, where sqrt(D) is a power of two, that the float64
    autograd reference is representable in fp32; the ratios to 2^24 are printed."""
    cs, e = PK.case(name), PK.expected(name)
    print(name, {k: round(v, 4) for k, v in PK.RATIO[name].items()})
    assert set(PK.RATIO[name]) == {'levels', 'grad_fmap1', 'grad_fmap2'} and max(PK.RATIO[name].values()) < 1.0
    assert e.exact == (cs.D in (4, 16, 64, 256)) and (e.b1 is None) == e.exact == (e.b2 is None)
    for t in [cs.f1, cs.f2] + cs.cot:
        assert t.dtype == torch.float32 and torch.equal(t, t.round())
    assert float(cs.f1.abs().max()) == 2 == float(cs.f2.abs().max()) and all(float(c.abs().max()) == 1 for c in cs.cot)
    scale = 4.0 ** (cs.L - 1)
    for lv in e.levels:
        assert lv.dtype == torch.float32 and bool(torch.isfinite(lv).all()) and float(lv.abs().max()) > 0
        if e.exact:                                           # a multiple of 4^-(L-1) / sqrt(D)
            v = lv.double() * PK.sqrt32(cs.D) * scale
            assert torch.equal(v, v.round())
    assert float(e.g1.abs().max()) > 0 and float(e.g2.abs().max()) > 0


@pytest.mark.parametrize('name', sorted(PK.MISSING))
def test_the_reference_without_a_level_is_the_sum_of_the_other_levels(name):
    """Linearity: the gradients with every cotangent are those without the missing levels plus those of the missing levels alone."""
    miss, _ = PK.MISSING[name]
    cs, full, part = PK.case(name), PK.expected(name), PK.expected(name, miss)
    rest = PK.expected(name, tuple(l for l in range(cs.L) if l not in miss))
    assert full.exact and torch.equal(part.g1.double() + rest.g1.double(), full.g1.double())
    assert torch.equal(part.g2.double() + rest.g2.double(), full.g2.double())
    assert not torch.equal(part.g1, full.g1) and not torch.equal(part.g2, full.g2)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PK.CASES)
def test_plan_model_against_the_library(name):
    """The forward workspace is the pooled feature maps (16 bytes at the least: the library never reports an empty workspace), the
    backward one 4 * (pooled + S1 * gP + (S > 1) * S * B * D * hw) with the table's S1 and S."""
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    cs = PK.case(name)
    P = PK.plan(cs)
    assert (P.S1, P.S) == (cs.S1, cs.S), (name, P.S1, P.S)
    assert P.pitch == [(v + 3) // 4 * 4 for v in cs.N] and P.kblocks == sum(n * ((v + 31) // 32) for n, v in zip(P.n, cs.N))
    desc = _desc(cs)
    assert L.mpc_corr_pyramid_supported(ctypes.byref(desc), cs.D) == 0
    assert L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(desc), cs.D, 0) == max(16, 4 * P.pooled)
    assert (P.pooled == 0) == (cs.L == 1)
    want = 4 * (P.pooled + cs.S1 * P.gp + (cs.S * cs.B * cs.D * cs.hw if cs.S > 1 else 0))
    assert L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(desc), cs.D, 1) == want == 4 * P.total_bwd
    print(f'{name}: S1 {P.S1} S {P.S} kblocks {P.kblocks} pitches {P.pitch} forward {4 * P.pooled} B backward {want} B')


def test_plan_of_the_named_figures():
    six, sixteen = PK.plan(PK.case('six_levels')), PK.plan(PK.case('sixteen'))
    assert PK.case('six_levels').N == [1665, 396, 99, 20, 4, 1] and six.kblocks == 210 and 3 * 53 == 159      # 53 k blocks of i
    assert (53 + six.S1 - 1) // six.S1 != 53 // six.S1                                          # 13 uneven ranges
    assert sixteen.kblocks == 543 and PK.case('sixteen').T == 16 == len(PK.case('sixteen').tix[0]) and PK.case('sixteen').L == 6
    for name, (miss, S) in PK.MISSING.items():
        assert PK.plan(PK.case(name), miss).S == S and PK.plan(PK.case(name), miss).S1 == PK.case(name).S1
    assert PK.MISSING['wide_l1'][1] == 1 and PK.MISSING['mixed'][1] == 6


# ---- the census -------------------------------------------------------------------------------------------------------------------
_TILED = {}


def _tiled(name, missing=(), mutant=None, aligned=True):
    key = (name, tuple(missing), mutant, aligned)
    if key not in _TILED:
        _TILED[key] = PK.tiled(name, missing, mutant, aligned)
    return _TILED[key]


# (product, operand,) item -> the cases named for it.  fwd: A = fmap1 (cp_load<false>), B = P_l (cp_load<false>); gP: A = fmap1
# (cp_load<true>), B = the cotangent (cp_load<false>); g1: A = P_l, B = the cotangent (both cp_load<true>).
REACHES = {
    ('fwd', 'A', 'interior'): ['interior', 'mixed', 'd256'], ('fwd', 'B', 'interior'): ['interior', 'mixed', 'wide_l1'],
    ('gP', 'A', 'interior'): ['d256', 'd160', 'd132', 'd512'], ('gP', 'B', 'interior'): ['interior', 'mixed', 'd256'],
    ('g1', 'A', 'interior'): ['d256', 'd160', 'd132', 'd512'], ('g1', 'B', 'interior'): ['interior', 'mixed', 'd256'],
    ('fwd', 'A', 'vec_ragged'): ['mixed', 'wide_l1'], ('fwd', 'B', 'vec_ragged'): ['mixed', 'interior'],
    ('gP', 'A', 'vec_ragged'): ['interior', 'd160'], ('gP', 'B', 'vec_ragged'): ['mixed'],
    ('g1', 'A', 'vec_ragged'): ['mixed', 'd160'], ('g1', 'B', 'vec_ragged'): ['mixed', 'wide_l1'],
    ('fwd', 'B', 'tail16'): ['mixed', 'six_levels', 'sixteen'], ('g1', 'A', 'tail16'): ['mixed', 'six_levels', 'sixteen'],
    ('fwd', 'A', 'scalar'): ['six_levels'], ('fwd', 'B', 'scalar'): ['six_levels'],
    ('gP', 'A', 'scalar'): ['six_levels'], ('gP', 'B', 'scalar'): ['six_levels', 'mixed'],
    ('g1', 'A', 'scalar'): ['six_levels'], ('g1', 'B', 'scalar'): ['six_levels', 'mixed'],
    ('fwd', 'm_rem'): ['mixed', 'wide_l1', 'six_levels'], ('fwd', 'n_rem'): ['mixed', 'six_levels'], ('fwd', 'k_rem'): ['d132', 'd8', 'six_levels'],
    ('gP', 'm_rem'): ['interior', 'd160', 'd132'], ('gP', 'n_rem'): ['mixed', 'six_levels'], ('gP', 'k_rem'): ['mixed', 'd132', 'six_levels'],
    ('g1', 'm_rem'): ['interior', 'd160', 'd132'], ('g1', 'n_rem'): ['mixed', 'six_levels'], ('g1', 'k_rem'): ['mixed', 'six_levels'],
    ('gP', 'm_rem_late'): ['d160', 'd132'], ('g1', 'm_rem_late'): ['d160', 'd132'],
    ('fwd', 'n_tiles_above_0'): ['wide_l1', 'six_levels'], ('gP', 'n_tiles_above_0'): ['wide_l1', 'six_levels'],
    ('gP', 'split'): ['interior', 'mixed', 'wide_l1', 'd8', 'six_levels', 'sixteen'], ('gP', 'uneven_ranges'): ['six_levels', 'sixteen'],
    ('g1', 'split'): ['interior', 'mixed', 'six_levels'], ('g1', 'split_cap'): ['six_levels', 'sixteen'],
    ('g1', 'uneven_ranges'): ['mixed', 'six_levels', 'sixteen'],
    ('g1', 'range_ends_in_ragged_block'): ['mixed', 'd132'], ('gP', 'range_ends_in_ragged_block'): ['mixed', 'six_levels'],
    ('g1', 'level_1x1'): ['six_levels', 'sixteen'], ('gather', 'level_1x1'): ['six_levels', 'sixteen'],
    ('gather', 'V4'): ['interior', 'mixed'], ('gather', 'V4_partials'): ['sixteen', 'mixed'], ('gather', 'V1'): ['six_levels'],
}
# what no shape can reach.  gP reads fmap1 along k = i with pitch hw and the cotangent with pitch N: `vec` needs the pitch to be a
# multiple of 4, and then the extent is one too, so a 16-byte load never has a tail there.  The n of grad_fmap1 is i: its tiles do
# not belong to a level.  fmap1 is the forward's only operand along m: no 16-byte tail without hw % 4 != 0, which clears `vec`.
NEVER = [('gP', 'A', 'tail16'), ('gP', 'B', 'tail16'), ('fwd', 'A', 'tail16'), ('g1', 'B', 'tail16'), ('g1', 'n_tiles_above_0')]


def test_the_cases_reach_what_the_table_claims():
    reached = {}
    for name in PK.CASES:
        for p in _tiled(name).paths:
            reached.setdefault(p, []).append(name)
    for item, names in REACHES.items():
        assert names and set(names) <= set(reached.get(item, ())), (item, names, reached.get(item))
    for item in NEVER:
        assert item not in reached, (item, reached.get(item))
    assert set(reached) == set(REACHES), set(reached) ^ set(REACHES)         # nothing is taken that the table does not name
    for item in sorted(reached):
        print(item, reached[item])
    # every tile of `interior`'s forward is interior, over two full k blocks; level 1 has N = 64
    paths = _tiled('interior').paths
    assert ('fwd', 'A', 'vec_ragged') not in paths and ('fwd', 'm_rem') not in paths and ('fwd', 'k_rem') not in paths
    assert PK.case('interior').D == 2 * PK.BK and PK.case('interior').N == [256, 64]
    # the production D: two interior m tiles in both backward products, nothing ragged in m
    paths = _tiled('d256').paths
    assert not {('gP', 'm_rem'), ('g1', 'm_rem'), ('gP', 'A', 'vec_ragged')} & paths
    assert PK.case('mixed').N == [240, 60, 15] and PK.plan(PK.case('mixed')).pitch == [240, 60, 16]
    assert PK.case('wide_l1').N == [576, 144] and PK.case('d132').D % PK.BK == 4 and PK.case('d160').D - PK.BM == 32 and PK.case('d512').D == 512
    assert PK.case('d8').D < PK.BK and not PK.pow2_scale(8) and not PK.pow2_scale(160) and PK.pow2_scale(256)


def test_a_missing_cotangent_under_a_split():
    for name in ('mixed', 'six_levels'):
        miss, S = PK.MISSING[name]
        r = _tiled(name, miss)
        assert S > 1 and ('g1', 'missing_cotangent_split') in r.paths and r.plan.S == S
    r = _tiled('wide_l1', PK.MISSING['wide_l1'][0])                      # the pooled operand alone, one range: no reduce launch
    assert r.plan.S == 1 and ('g1', 'split') not in r.paths and ('g1', 'A', 'interior') not in r.paths
    assert all(('g1', 'missing_cotangent_split') not in _tiled(n).paths for n in PK.CASES)


def test_alignment_alone_decides_the_loader_of_offset():
    cs = PK.case('offset')
    assert cs.hw == 128 and cs.w % 4 == 0 and all(v % 4 == 0 for v in cs.N) and PK.GUARD_CASES == ('mixed', 'six_levels', 'offset')
    on, off = _tiled('offset').paths, _tiled('offset', aligned=False).paths
    loads = lambda paths: {p for p in paths if len(p) == 3}             # noqa: E731
    assert all(p[2] in ('interior', 'vec_ragged') for p in loads(on)) and ('gather', 'V4') in on
    # shifted by one float only the pooled operand (the aligned workspace) is still read 16 bytes at a time
    assert {p for p in loads(off) if p[2] != 'scalar'} == {('fwd', 'B', 'vec_ragged'), ('g1', 'A', 'vec_ragged')} and ('gather', 'V1') in off
    for o in ('A', 'B'):
        assert all((prod, o, 'scalar') in off for prod in ('fwd', 'gP', 'g1'))
    a, b = _tiled('offset'), _tiled('offset', aligned=False)
    assert torch.equal(a.g1, b.g1) and torch.equal(a.g2, b.g2) and all(torch.equal(x, y) for x, y in zip(a.levels, b.levels))


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def _check(name, missing=(), mutant=None):
    r = _tiled(name, missing, mutant)
    label = name if mutant is None else f'{name} [{mutant}]'
    PK.compare_all(label, name, missing, levels=None if missing else r.levels, g1=r.g1, g2=r.g2)


@pytest.mark.parametrize('name', PK.CASES)
def test_the_restated_tiling_passes(name):
    """Every block of the three products writes its tile, and nothing is left unwritten (the restatement starts from NaN)."""
    _check(name)
    if name in PK.MISSING:
        _check(name, PK.MISSING[name][0])


# mutant -> the output that names the first bad element and exactly the cases that catch it
CAUGHT = {
    'drop_last_kblock': ('grad_fmap1', set(PK.CASES)),
    'first_partial_only': ('grad_fmap2', {'interior', 'mixed', 'wide_l1', 'd8', 'six_levels', 'sixteen'}),          # S1 > 1
    'slot_as_target': ('level_[12]', {'mixed', 'd132', 'six_levels', 'sixteen'}),                                # a level that skips a target
    'pitch_as_n': ('level_[25]', {'mixed', 'six_levels', 'sixteen'}),                                            # N_l % 4 != 0 above level 0
    'no_width_test': ('grad_fmap2', {'six_levels'}),                                                             # a level that drops a column
    'sample_slot_swapped': ('level_0', {'mixed', 'd132', 'offset'}),                                             # B > 1 and T > 1
}


def test_every_named_mutant_is_listed():
    assert set(CAUGHT) == set(PK.MUTANTS) and len(PK.MUTANTS) == 6


@pytest.mark.parametrize('mutant', PK.MUTANTS)
def test_mutants_fail_the_comparator_on_their_cases_and_on_no_other(mutant):
    """A split range that drops its last k block, the gather ignoring the partials s >= 1, slot k of a level above 0 read as target
    k, the pooled pitch used as N, (x + u) >> l clamped instead of tested against w_l, sample and slot swapped in a volume's row
    offset."""
    where, names = CAUGHT[mutant]
    for name in PK.CASES:
        if name in names:
            with pytest.raises(AssertionError, match='first bad element') as e:
                _check(name, mutant=mutant)
            assert re.search(rf'^{name} \[{mutant}\] {where}: first bad element \((level \d, slot \d+, sample \d+, i \d+, j \d+|t, b, c, y, x\) = \([-\d]+(, \d+){{4}})\): '
                             r'got \S+, expected \S+', str(e.value)), str(e.value)
        else:
            _check(name, mutant=mutant)


def test_a_mutant_corrupts_the_elements_it_should():
    """The unclamped width test differs only in the column a level drops; the gather's first partial alone leaves grad_fmap1 as it was."""
    cs, e = PK.case('six_levels'), PK.expected('six_levels')
    bad = _tiled('six_levels', mutant='no_width_test').g2 != e.g2
    kept = min((cs.w >> l) << l for l in range(cs.L))                   # 32: levels 4 and 5 stop there, level 1 at 44
    assert kept == 32 and bool(bad[..., cs.w - 1].any()) and bool(bad[..., kept].any()) and not bool(bad[..., :kept].any())
    r = _tiled('sixteen', mutant='first_partial_only')
    assert torch.equal(r.g1, PK.expected('sixteen').g1) and all(torch.equal(a, b) for a, b in zip(r.levels, PK.expected('sixteen').levels))


def test_the_comparator_refuses_a_nan_and_a_flipped_sign_of_zero():
    want = torch.zeros(1, 2, 1, 1, 2)
    PK.compare('zeros', 'level_0', torch.zeros(1, 2, 1, 1, 2), want, B=2)
    with pytest.raises(AssertionError, match=r'first bad element \(level 0, slot 0, sample 1, i 0, j 1\)'):
        PK.compare('zeros', 'level_0', torch.tensor([0.0, 0.0, 0.0, -0.0]).reshape(1, 2, 1, 1, 2), want, B=2)
    with pytest.raises(AssertionError, match=r'first bad element \(t, b, c, y, x\) = \(-, 0, 1, 0, 0\)'):
        PK.compare('bounded', 'grad_fmap1', torch.tensor([0.0, float('nan')]).reshape(1, 2, 1, 1), torch.zeros(1, 2, 1, 1, dtype=torch.float64),
                   torch.ones(1, 2, 1, 1, dtype=torch.float64))
    book = {}
    PK.compare('a', 'grad_fmap2', torch.ones(1, 1, 1, 1, 2), torch.ones(1, 1, 1, 1, 2), book=book)
    PK.compare('b', 'grad_fmap2', torch.ones(1, 1, 1, 1, 2), torch.ones(1, 1, 1, 1, 2, dtype=torch.float64) * 1.5, torch.ones(1, 1, 1, 1, 2, dtype=torch.float64), book=book)
    assert book == {'grad_fmap2': [2, 4, 2, 0.5, 'b']}
