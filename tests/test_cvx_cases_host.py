"""The convex-upsampling cases of tests/cvx_cases.py on the CPU: the exactness precondition of every case, the float64 formula and
the thread-by-thread restatement of the four kernels against the float64 autograd result through the plain-torch mirror of
utils/basis.py (bit for bit, nothing left NaN), what the named cases claim to reach (a census taken while the restatement walks the
threads), the workspace sizes of the library, and the comparator itself: eleven named mutants of the restatement fail it with an
assertion that names the first bad element, on exactly the cases listed."""
import re

import pytest
import torch

import cvx_cases as CK

ALL = CK.CASES + (CK.LARGE,)


# ---- preconditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_every_sum_is_exact_and_the_reference_representable(name):
    """expected() asserts A / UNIT < 2^24 for every output, every value a multiple of its UNIT and representable in fp32; the ratios
    to 2^24 are printed.  The inputs are what the module says: logits 0 or -1000 with 1, 2, 4 or 8 zeros a pixel, integers, eighths."""
    cs, e = CK.case(name), CK.expected(name)
    print(name, {k: round(v, 5) for k, v in CK.RATIO[name].items()})
    assert set(CK.RATIO[name]) == set(CK.OUTPUTS) and max(CK.RATIO[name].values()) < 1.0
    zeros = (cs.mask.reshape(cs.B, 9, 8, 8, cs.h, cs.w) == 0)
    assert bool(((cs.mask == 0) | (cs.mask == -1000)).all()) and cs.mask.dtype == torch.float32
    m = zeros.sum(dim=1)
    assert set(m.unique().tolist()) == ({1} if name == 'onehot_border' else {1, 2, 4, 8})
    w = CK.softmax64(cs.mask)
    assert torch.equal(w, zeros.double() / m[:, None].double())                       # every weight is 0 or exactly 1 / m
    assert torch.equal(torch.softmax(cs.mask.reshape(cs.B, 9, 8, 8, cs.h, cs.w), dim=1).double(), w)
    for t, top in ((cs.params, 3), (cs.g, 2), (cs.basis * 8, 8)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and (t.numel() == 0 or float(t.abs().max()) <= top)
    assert cs.scale == 0.5 and torch.equal(cs.pos, torch.nonzero(_tile_mask(cs)))
    for k in CK.OUTPUTS:
        assert getattr(e, k).dtype == torch.float32 and bool(torch.isfinite(getattr(e, k)).all())
    if cs.n:
        assert all(float(getattr(e, k).abs().max()) > 0 for k in CK.OUTPUTS if not (k == 'grad_mask' and name == 'onehot_border'))
    else:
        assert e.traj.numel() == 0 == e.dflow.numel() and float(e.grad_mask.abs().max()) == 0 == float(e.grad_params.abs().max())


def _tile_mask(cs):
    from motionpriorcmax_amd import utils
    return utils.get_optical_flow_tile_mask((8 * cs.h, 8 * cs.w), cs.tile)


def test_the_shapes_are_what_the_table_says():
    c = CK.case
    assert c('tile1_row').n == 448 and c('tile3').ntx == 13 and 8 * c('tile3').w % 3 and c('tile5_d11').T * c('tile5_d11').d == 264
    assert c('tile16_d16').T * c('tile16_d16').d == 528 and 8 * c('tile16_d16').h % 16 and c('tile16_d16').n == 2
    assert c('tile32_one').n == 1 and c('tile32_one').pos.tolist() == [[16, 16]] and c('tile32_none').n == 0
    assert c('plane1025_t4').plane == 1025 == CK.FILL_ELEMS + 1 and c('plane2052_t4').plane == 2052 == 2 * CK.FILL_ELEMS + 4
    assert c(CK.LARGE).plane == 4800 and c('onehot_border').n == 24 and (c('plane1025_t4').n % 256, c('plane1025_t16').n % 256) == (4, 240)


# ---- the references agree ---------------------------------------------------------------------------------------------------------
_RESTATED = {}


def _restated(name, mutant=None):
    if (name, mutant) not in _RESTATED:
        _RESTATED[name, mutant] = CK.restated(name, mutant)
    return _RESTATED[name, mutant]


def _check(name, mutant=None):
    r = _restated(name, mutant)
    label = name if mutant is None else f'{name} [{mutant}]'
    CK.compare_all(label, name, **{k: getattr(r, k) for k in CK.OUTPUTS})


@pytest.mark.parametrize('name', ALL)
def test_the_formula_and_the_restatement_equal_float64_autograd(name):
    """traj, flows and both gradients of the mirror in float64 -- autograd, no formula of this module -- against `evaluate` and
    against `restated`, which starts from NaN: every element is written, by exactly one role of the backward (asserted inside)."""
    cs, e, r = CK.case(name), CK.expected(name), _restated(name)
    a = CK.autograd64(cs)
    for k in ('traj', 'flows', 'grad_params', 'grad_mask'):
        assert getattr(a, k).dtype == torch.float64 and torch.equal(getattr(a, k), getattr(e, k).double()), (name, k)
    for k in CK.OUTPUTS:
        assert not bool(torch.isnan(getattr(r, k)).any()), (name, k)
    _check(name)
    # the store form follows the address alone: one float off a 16-byte boundary the same bits
    off = CK.restated(name, base_offset=1)
    assert all(torch.equal(getattr(off, k), getattr(r, k)) for k in CK.OUTPUTS)


def test_the_workspace_sizes_of_the_library():
    """mpc_cvx_traj_bwd_workspace_bytes: (2d + 9) floats a centre, rounded up to 256 bytes; no centre, an aligned 0."""
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    for name in ALL:
        cs = CK.case(name)
        want = -(-cs.B * cs.n * (2 * cs.d + 9) * 4 // 256) * 256
        assert L.mpc_cvx_traj_bwd_workspace_bytes(cs.B, cs.d, cs.T, cs.h, cs.w, cs.tile) == want, name
    cs = CK.case('tile32_none')
    assert L.mpc_cvx_traj_bwd_workspace_bytes(cs.B, cs.d, cs.T, cs.h, cs.w, cs.tile) == 0


# ---- the census -------------------------------------------------------------------------------------------------------------------
_PAD = [('pad', side, k) for side, ks in (('top', (0, 1, 2)), ('bottom', (6, 7, 8)), ('left', (0, 3, 6)), ('right', (2, 5, 8))) for k in ks]
REACHES = {
    'fill_float4_store': ['onehot_border', 'tile2', 'plane1025_t4', 'plane1025_t16', 'plane2052_t4'],
    'fill_scalar_store': ['onehot_border', 'tile3', 'plane1025_t4', 'plane1025_t16'],
    'fill_chunk_above_0': ['plane1025_t4', 'plane1025_t16', 'plane2052_t4'],
    'fill_uni_early_return': ['onehot_border', 'tile1_row', 'tile2', 'tile8', 'plane1025_t4', 'plane2052_t4'],
    'fill_per_element_quad_with_a_centre': ['tile3', 'tile5_d11', 'tile16_d16', 'tile32_one', 'plane1025_t16'],
    'fill_per_element_quad_without_a_centre': ['tile3', 'tile5_d11', 'tile16_d16', 'tile32_one', 'tile32_none', 'plane1025_t16'],
    ('basis_passes', 1): ['onehot_border', 'tile1_row'], ('basis_passes', 2): ['tile5_d11'], ('basis_passes', 3): ['tile16_d16'],
    ('template', 4, 1): ['plane1025_t4', 'plane1025_t16', 'plane2052_t4'], ('template', 4, 4): ['tile8', 'tile32_one', 'tile32_none'],
    ('template', 10, 5): ['tile3'], ('template', 10, 10): ['tile1_row'], ('template', 16, 11): ['tile5_d11'], ('template', 16, 16): ['tile16_d16'],
    ('centres_in_a_cell', 0): ['tile16_d16', 'tile32_one', 'tile32_none', 'plane1025_t16'],
    ('centres_in_a_cell', 1): ['tile8', 'tile5_d11', 'tile16_d16', 'tile32_one', 'plane1025_t16'],
    ('centres_in_a_cell', 'several'): ['onehot_border', 'tile1_row', 'tile2', 'tile3', 'tile5_d11', 'plane1025_t4'],
    'gather_range_empty': ['tile16_d16', 'tile32_one', 'plane1025_t16'],
    'workgroup_spans_two_samples': ['onehot_border', 'tile1_row', 'tile3', 'plane1025_t4', 'plane1025_t16'],
}
REACHES.update({p: ['onehot_border', 'tile1_row'] for p in _PAD})
OTHER = {('template', 4, 2), ('template', 4, 3)}            # taken by cases that are named for something else


def test_the_cases_reach_what_the_table_claims():
    reached = {}
    for name in CK.CASES:
        for p in _restated(name).census:
            reached.setdefault(p, []).append(name)
    for item in sorted(reached, key=str):
        print(item, reached[item])
    for item, names in REACHES.items():
        assert names and set(names) <= set(reached.get(item, ())), (item, names, reached.get(item))
    assert set(reached) == set(REACHES) | OTHER, set(reached) ^ (set(REACHES) | OTHER)
    # what single cases are in the table for
    census = lambda name: _restated(name).census                                    # noqa: E731
    assert 'fill_chunk_above_0' not in census('tile16_d16') and 'fill_float4_store' in census('plane2052_t4') and 'fill_scalar_store' not in census('plane2052_t4')
    assert 'workgroup_spans_two_samples' in census('tile1_row') and CK.case('tile1_row').n > 256 and CK.case('tile1_row').n % 256
    assert 'fill_uni_early_return' not in census('tile3') and ('pad', 'top', 1) in census('tile1_row') and ('pad', 'bottom', 7) in census('tile1_row')
    assert ('centres_in_a_cell', 'several') not in census('tile32_one') and ('centres_in_a_cell', 1) not in census('tile32_none')
    big = census(CK.LARGE)                                   # the workload's plane adds chunk counts, no path
    assert big <= set(reached) and 'fill_chunk_above_0' in big


def test_the_gather_clip_to_the_grid_never_binds():
    """min(.., nty - 1) in k_cvx_bwd_params: a cell of the grid ends at 8 cy + 7 <= 8 h - 1, and floor((8 h - 1 - s) / tile) is
    cvx_tiles(8 h, tile) - 1, so the clip that matters is the one to the cell's last row -- which the mutant gather_hi_unclipped drops."""
    for tile in range(1, 41):
        s = tile >> 1
        for h in range(1, 12):
            nt = CK.tiles(8 * h, tile)
            for cy in range(h):
                if 8 * cy + 7 < s:
                    continue
                assert (8 * cy + 7 - s) // tile <= nt - 1, (tile, h, cy)
            assert nt == len(range(s, 8 * h, tile))


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def _caught(first, names, **other):
    return {**{n: first for n in names}, **other}


_EVEN = ['onehot_border', 'tile2', 'tile8', 'tile16_d16', 'tile32_one', 'plane1025_t4', 'plane1025_t16', 'plane2052_t4']
_WITH_CENTRES = [n for n in CK.CASES if n != 'tile32_none']
# mutant -> the cases that catch it, each with the first output (in the order of OUTPUTS) that names a bad element
CAUGHT = {
    'k_transposed': _caught('traj', _WITH_CENTRES, tile32_none='flows'),
    'pad_clamped': _caught('traj', _WITH_CENTRES, tile32_one='flows', tile32_none='flows', plane1025_t16='flows'),
    'sy_sx_swapped': _caught('traj', _WITH_CENTRES, tile8='flows', tile16_d16='flows', tile32_one='flows', tile32_none='flows', plane1025_t16='flows'),
    'xy_swapped': _caught('traj', _WITH_CENTRES, tile32_none='flows'),
    'centre_floor': _caught('traj', _EVEN, tile32_none='grad_mask'),                      # an even tile; odd tiles and tile 1 have (tile - 1) / 2 = tile / 2
    'gather_same_k': _caught('grad_params', _WITH_CENTRES),
    'gather_hi_unclipped': _caught('grad_params', [n for n in _WITH_CENTRES if n != 'tile32_one']),        # more than one centre
    'fill_first_chunk_only': _caught('grad_mask', ['plane1025_t4', 'plane1025_t16', 'plane2052_t4']),      # a plane above 1024 cells
    'fill_uni_always': _caught('grad_mask', ['tile3', 'tile5_d11', 'tile16_d16', 'tile32_one', 'plane1025_t16']),       # 8 % tile != 0 and a centre
    'basis_first_256': _caught('traj', ['tile5_d11', 'tile16_d16']),                      # T * d > 256
    'sample_stride_n_rounded': _caught('traj', ['onehot_border', 'tile1_row', 'tile3', 'plane1025_t4', 'plane1025_t16']),   # B > 1, n % 256 != 0
}


def test_every_named_mutant_is_listed():
    assert set(CAUGHT) == set(CK.MUTANTS) and len(CK.MUTANTS) == 11 and all(CAUGHT.values())


@pytest.mark.parametrize('mutant', CK.MUTANTS)
def test_mutants_fail_the_comparator_on_their_cases_and_on_no_other(mutant):
    """Neighbour k read as (k % 3, k / 3); the border clamped in place of zero-padded; the channel as sx * 8 + sy; the x and y halves
    of params exchanged; centres at (tile - 1) / 2; the params gather reading w_k of the cell at +k in place of -k; its ranges not
    clipped to the cell's last row and column; the zero fill only in chunk 0; the fill's `uni` shortcut for every tile; only the first
    256 elements of the basis staged; b decoded as if n were padded to a multiple of 256."""
    for name in CK.CASES:
        if name in CAUGHT[mutant]:
            with pytest.raises(AssertionError, match='first bad element') as e:
                _check(name, mutant)
            assert re.search(rf'^{name} \[{mutant}\] {CAUGHT[mutant][name]}: first bad element \(\d+(, \d+)*\): got \S+, expected \S+', str(e.value)), str(e.value)
        else:
            _check(name, mutant)


def test_a_mutant_corrupts_the_elements_it_should():
    """The clamped border differs from the zero padding only where a selected neighbour is padding; the fill that stops after chunk
    0 leaves exactly the elements from 1024 on unwritten, in the planes that are no centre's."""
    cs, e = CK.case('onehot_border'), CK.expected('onehot_border')
    bad = (_restated('onehot_border', 'pad_clamped').flows != e.flows).any(dim=0).any(dim=1)               # [B, 8h, 8w]
    sel = (cs.mask.reshape(cs.B, 9, 8, 8, cs.h, cs.w) == 0).permute(0, 1, 4, 2, 5, 3).reshape(cs.B, 9, 8 * cs.h, 8 * cs.w).float().argmax(dim=1)
    cy, cx = torch.arange(8 * cs.h)[:, None] // 8, torch.arange(8 * cs.w)[None] // 8
    ny, nx = cy + sel // 3 - 1, cx + sel % 3 - 1
    outside = (ny < 0) | (ny >= cs.h) | (nx < 0) | (nx >= cs.w)
    assert bool(bad.any()) and not bool((bad & ~outside).any())
    cs, e = CK.case('plane1025_t4'), CK.expected('plane1025_t4')
    gm = _restated('plane1025_t4', 'fill_first_chunk_only').grad_mask.reshape(cs.B, 576, cs.plane)
    hole = torch.isnan(gm)
    assert not bool(hole[..., :1024].any()) and int(hole[..., 1024].sum()) == cs.B * 9 * 60 and torch.equal(gm[~hole], e.grad_mask.reshape(cs.B, 576, -1)[~hole])


def test_the_comparator_takes_either_zero_and_refuses_a_nan():
    want = torch.zeros(2, 3)
    CK.compare('zeros', 'traj', torch.tensor([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0]]), want)
    with pytest.raises(AssertionError, match=r'zeros traj: first bad element \(1, 2\): got nan, expected 0.0 \(1 of 6 bad\)'):
        CK.compare('zeros', 'traj', torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, float('nan')]]), want)
    want64, bound = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([0.5, 0.0], dtype=torch.float64)
    assert CK.compare('bounded', 'flows', torch.tensor([1.25, 0.0]), want64, bound) == 0.5
    with pytest.raises(AssertionError, match=r'first bad element \(1,\)'):                 # a bound of 0 asks for exactly 0
        CK.compare('bounded', 'flows', torch.tensor([1.0, 1e-30]), want64, bound)
    with pytest.raises(AssertionError, match=r'first bad element \(0,\)'):
        CK.compare('bounded', 'flows', torch.tensor([float('nan'), 0.0]), want64, bound)


def test_the_counted_roundings():
    """N_X of roundings(), spelt out for the workload's d = 10, T = 8 at tile 4 and for the extremes of the table."""
    cs = CK.make_case('x', 1, 10, 1, 1, 4, 8, torch.zeros(1, 20, 1, 1), torch.zeros(1, 576, 1, 1), torch.zeros(8, 10), torch.zeros(1, 8, 4, 2), 1.0)
    assert CK.roundings(cs) == dict(flows=20, traj=21, dflow=9, grad_mask=40, grad_params=45)
    assert CK.roundings('tile1_row')['grad_params'] == 9 + 9 * 64 and CK.roundings('tile16_d16') == dict(flows=26, traj=27, dflow=34, grad_mask=77, grad_params=43)
    assert CK.gamma(1) > CK.U and abs(CK.gamma(45) / (45 * CK.U) - 1) < 1e-5
