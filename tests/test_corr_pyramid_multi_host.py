"""The correlation pyramid over several references (events plus frames) on the host: the list form of utils.corr_pyramid -- the
plain-torch mirror, written as the reference's expand / cat, batched matmul, division and pools -- against the g23 fixtures of the
unmodified reference (tools/gen_golden_corr_multi.py), against the tensor form per reference, and on the exact cases of
tests/corr_pyramid_multi_cases.py; the routing of utils.corr_pyramid_fused / CorrLookup.from_fmaps for lists the kernels do not take;
and the host-only part of the C ABI (include/mpcmax.h: mpc_corr_pyramid_multi_*)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
import corr_pyramid_cases as PK
import corr_pyramid_multi_cases as MK

NAMES = ('mpc_corr_pyramid_multi_workspace_bytes', 'mpc_corr_pyramid_multi_supported', 'mpc_corr_pyramid_multi_fwd',
         'mpc_corr_pyramid_multi_bwd')
G23 = ('a', 'b')
MAPS = ('fmap1_events', 'fmap1_frames', 'fmap2_events', 'fmap2_frames')


def fixture(case):
    g = load_golden('g23_corr_multi_' + case)
    f1 = [torch.from_numpy(g['fmap1_events']), torch.from_numpy(g['fmap1_frames'])]
    f2 = [torch.from_numpy(g['fmap2_events']), torch.from_numpy(g['fmap2_frames'])]
    nls = [[int(v) for v in g['num_levels_events']], [int(v) for v in g['num_levels_frames']]]
    L = max(max(v) for v in nls)
    return g, f1, f2, nls, L


# ---- 1. the mirror against the fixtures
@pytest.mark.parametrize('case', G23)
def test_the_list_form_mirror_gives_the_fixture_bit_for_bit(case):
    from motionpriorcmax_amd import utils
    g, f1, f2, nls, L = fixture(case)
    a, b = [t.clone().requires_grad_(True) for t in f1], [t.clone().requires_grad_(True) for t in f2]
    levels, tix = utils.corr_pyramid(a, b, nls)
    assert len(levels) == L and tix == [[int(v) for v in g[f'target_indices_{l}']] for l in range(L)]
    for l, lv in enumerate(levels):
        want = torch.from_numpy(g[f'level_{l}'])
        assert lv.dtype == torch.float32 and lv.shape == want.shape and torch.equal(lv, want), (case, l)
    grads = torch.autograd.grad(levels, a + b, [torch.from_numpy(g[f'cot_{l}']) for l in range(L)])
    for name, got in zip(MAPS, grads):
        assert torch.equal(got, torch.from_numpy(g['grad_' + name])), (case, name)
    # and through the lookup's constructor on the CPU: the same levels, the merged level counts
    lk = utils.CorrLookup.from_fmaps(f1, f2, nls, radius=int(g['radius']))
    assert lk.num_levels_per_target == nls[0] + nls[1] and lk.target_indices == tix
    assert all(torch.equal(x, y) for x, y in zip(lk.levels, levels))
    out = lk.lookup(torch.from_numpy(g['coords']))
    want = torch.from_numpy(g['out'])
    assert out.shape == want.shape and float((out - want).abs().max()) <= 4.0 * float(g['err_out'])


# ---- 2. the mirror against itself
@pytest.mark.parametrize('name', MK.CASES)
def test_the_list_form_is_the_tensor_form_per_reference_by_slot_range(name):
    from motionpriorcmax_amd import utils
    cs = MK.case(name)
    levels, tix = utils.corr_pyramid(cs.f1, cs.f2, cs.nls)
    assert tix == cs.tix == utils.level_target_indices(cs.nl)
    alone = [utils.corr_pyramid(cs.f1[r], cs.f2[r], cs.nls[r])[0] for r in range(cs.R)]
    for l, (lv, want) in enumerate(zip(levels, MK.merge(cs, alone))):
        assert tuple(lv.shape) == (len(cs.tix[l]), cs.B * cs.hw, 1, cs.h >> l, cs.w >> l) and torch.equal(lv, want), (name, l)
    for r in range(cs.R):
        for l in range(len(alone[r])):
            s0, n = MK.slots(cs, r, l)
            assert n == alone[r][l].shape[0] and torch.equal(levels[l][s0:s0 + n], alone[r][l])


def test_a_list_of_one_reference_is_the_tensor_form():
    from motionpriorcmax_amd import utils
    gen = torch.Generator().manual_seed(5)
    f1, f2 = torch.randn(2, 12, 6, 7, generator=gen), torch.randn(3, 2, 12, 6, 7, generator=gen)
    want, wtix = utils.corr_pyramid(f1, f2, [2, 1, 2])
    for fn in (utils.corr_pyramid, utils.corr_pyramid_fused):
        for form in (([f1], [f2], [[2, 1, 2]]), ((f1,), (f2,), ([2, 1, 2],))):
            got, tix = fn(*form)
            assert tix == wtix and all(torch.equal(x, y) for x, y in zip(got, want))
    got, tix = utils.corr_pyramid([f1], [f2[0]], [2])                      # one target as 4 dimensions, its level count an int
    assert tix == [[0], [0]] and torch.equal(got[1], utils.corr_pyramid(f1, f2[0], 2)[0][1])


# ---- 3. the exact cases
@pytest.mark.parametrize('name', MK.CASES)
def test_the_exact_cases_meet_their_precondition_and_the_mirror_meets_them(name):
    from motionpriorcmax_amd import utils
    cs = MK.case(name)
    MK.expected(name)
    print(f'{name}: precondition ratios to 2^24: ' + '  '.join(f'{k} {v:.4f}' for k, v in MK.RATIO[name].items()))
    assert all(v < 1.0 for v in MK.RATIO[name].values())
    a, b = [t.clone().requires_grad_(True) for t in cs.f1], [t.clone().requires_grad_(True) for t in cs.f2]
    levels, _ = utils.corr_pyramid(a, b, cs.nls)
    grads = torch.autograd.grad(levels, a + b, cs.cot)
    e = MK.expected(name)
    MK.compare_all(f'{name} mirror', name, levels=levels if e.exact else levels[:1], g1=grads[:cs.R], g2=grads[cs.R:])
    for l in range(cs.L if e.exact else 1, cs.L):
        # sqrt(D) no power of two: the mirror pools the rounded quotients of level 0 (the kernels divide the pooled sum once) -- one
        # division and three additions per pool over exact sums: gamma(1 + 3 l + 8) * A
        PK.compare(f'{name} mirror', f'level_{l}', levels[l], e.levels64[l], PK.gamma(1 + 3 * l) * e.levels_abs[l], B=cs.B)


def test_the_cases_are_the_ones_the_kernels_can_go_wrong_at():
    cs = MK.case('three_ragged')
    assert cs.hw % 2 == 1 and not PK.pow2_scale(cs.D) and cs.R == 3
    cs = MK.case('sixteen')
    assert cs.R == 4 and cs.T == 16 and cs.L == 6
    cs = MK.case('stops_at_0')
    assert MK.slots(cs, 0, 1) == (0, 0) and MK.slots(cs, 1, 1) == (0, 1) and MK.slots(cs, 1, 0) == (2, 1)
    cs = MK.case('base_model')
    assert [MK.slots(cs, 1, l) for l in range(4)] == [(4, 1), (3, 1), (2, 1), (1, 1)]
    # both backward products split differently per reference somewhere: the per-reference plan is exercised
    plans = [MK.split_plan(cs, r) for r in range(cs.R)]
    assert len({(p.S1, p.S) for p in plans}) > 1, [(p.S1, p.S) for p in plans]


# ---- 4. missing cotangents and partial gradients (the mirror; the device in tests/test_gpu_corr_pyramid_multi.py)
@pytest.mark.parametrize('name', sorted(MK.MISSING))
def test_a_level_without_a_cotangent_is_a_missing_term_in_the_mirror(name):
    from motionpriorcmax_amd import utils
    cs, missing = MK.case(name), MK.MISSING[name]
    a, b = [t.clone().requires_grad_(True) for t in cs.f1], [t.clone().requires_grad_(True) for t in cs.f2]
    levels, _ = utils.corr_pyramid(a, b, cs.nls)
    keep = [l for l in range(cs.L) if l not in missing]
    grads = torch.autograd.grad([levels[l] for l in keep], a + b, [cs.cot[l] for l in keep], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, a + b)]
    MK.compare_all(f'{name} mirror without {list(missing)}', name, missing, g1=grads[:cs.R], g2=grads[cs.R:])


# ---- 5. the host-only ABI
def _desc(cs):
    from motionpriorcmax_amd import ops
    return ops.corr_pyramid_desc(cs.B, cs.h, cs.w, cs.nl)[0]


def test_header_declares_and_library_exports_the_entry_points():
    from motionpriorcmax_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert int(re.search(r'#define MPC_CORR_MAX_REFS (\d+)', header).group(1)) == _lib.CORR_MAX_REFS == 4
    assert ctypes.sizeof(_lib.CorrRefs) == 8 * (3 + 4 * _lib.CORR_MAX_REFS)


@pytest.mark.parametrize('name', MK.CASES)
def test_supported_and_workspace_agree_with_the_references_taken_alone(name):
    from motionpriorcmax_amd import ops, _lib
    L = _lib.lib()
    cs = MK.case(name)
    desc, refs = _desc(cs), ops.corr_pyramid_refs([len(v) for v in cs.nls])
    assert [refs.first_target[r] for r in range(cs.R + 1)] == cs.first
    assert L.mpc_corr_pyramid_multi_supported(ctypes.byref(desc), cs.D, ctypes.byref(refs)) == 0
    for backward in (0, 1):
        alone = 0
        for r in range(cs.R):
            d = ops.corr_pyramid_desc(cs.B, cs.h, cs.w, cs.nls[r])[0]
            assert L.mpc_corr_pyramid_supported(ctypes.byref(d), cs.D) == 0
            nb = L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(d), cs.D, backward)
            P = MK.split_plan(cs, r)
            assert nb == max(16, 4 * (P.total_bwd if backward else P.pooled))
            alone += nb
        assert L.mpc_corr_pyramid_multi_workspace_bytes(ctypes.byref(desc), cs.D, ctypes.byref(refs), backward) == alone


def test_what_the_multi_entry_points_refuse():
    from motionpriorcmax_amd import ops, _lib
    L = _lib.lib()
    cs = MK.case('base_model')
    desc = _desc(cs)

    def rcs(refs, D=cs.D):
        p = None if refs is None else ctypes.byref(refs)
        return (L.mpc_corr_pyramid_multi_supported(ctypes.byref(desc), D, p), L.mpc_corr_pyramid_multi_workspace_bytes(ctypes.byref(desc), D, p, 1),
                L.mpc_corr_pyramid_multi_fwd(ctypes.byref(desc), D, p, None, None), L.mpc_corr_pyramid_multi_bwd(ctypes.byref(desc), D, p, None, None))
    good = ops.corr_pyramid_refs([4, 1])
    assert rcs(good)[0] == 0 and rcs(good)[1] > 0
    assert rcs(good)[2] == _lib.E_NULL                                      # null tensors: refused on the host, nothing launched
    assert rcs(good)[3] == 0                                                # no gradient asked for: nothing to do
    assert rcs(None) == (_lib.E_NULL,) * 4
    many = _lib.CorrRefs(R=_lib.CORR_MAX_REFS + 1)
    assert rcs(many) == (_lib.E_UNSUPPORTED,) * 4 and b'references' in L.mpc_last_error_string()
    assert rcs(_lib.CorrRefs(R=0)) == (_lib.E_UNSUPPORTED,) * 4
    for counts in ([4], [3, 1], [4, 2], [4, 0, 1], [5, 0]):                 # short, short, long, an empty reference, twice
        bad = ops.corr_pyramid_refs(counts)
        assert rcs(bad) == (_lib.E_SHAPE,) * 4, counts
        assert b'first_target does not cover' in L.mpc_last_error_string()
    bad = ops.corr_pyramid_refs([4, 1])
    bad.first_target[0] = 1
    assert rcs(bad) == (_lib.E_SHAPE,) * 4
    assert rcs(good, D=6) == (_lib.E_UNSUPPORTED,) * 4 and b'multiple of 4' in L.mpc_last_error_string()


def test_unequal_shapes_and_mismatched_lists_raise_value_errors():
    from motionpriorcmax_amd import utils
    z = torch.zeros
    bad = [
        ([z(1, 4, 3, 4), z(1, 4, 3, 5)], [z(1, 1, 4, 3, 4), z(1, 1, 4, 3, 5)], [[1], [1]]),          # grids differ between references
        ([z(1, 4, 3, 4), z(1, 8, 3, 4)], [z(1, 1, 4, 3, 4), z(1, 1, 8, 3, 4)], [[1], [1]]),          # D differs
        ([z(1, 4, 3, 4), z(2, 4, 3, 4)], [z(1, 1, 4, 3, 4), z(1, 2, 4, 3, 4)], [[1], [1]]),          # batches differ
        ([z(1, 4, 3, 4), z(1, 4, 3, 4)], [z(1, 1, 4, 3, 4), z(2, 1, 4, 3, 4)], [[1], [1]]),          # two targets, one level count
        ([z(1, 4, 3, 4), z(1, 4, 3, 4)], [z(1, 1, 4, 3, 4)], [[1], [1]]),                            # lists of different lengths
        ([z(1, 4, 3, 4), z(1, 4, 3, 4)], [z(1, 1, 4, 3, 4), z(1, 1, 4, 3, 4)], [[1]]),
        ([z(1, 4, 3, 4), z(1, 4, 3, 4)], z(2, 1, 4, 3, 4), [[1], [1]]),                              # fmap2 not a list
        ([z(1, 4, 3, 4), z(1, 4, 3, 4)], [z(1, 1, 4, 3, 4), z(1, 1, 4, 3, 4)], [[1], [0]]),          # no level
        ([], [], []),
    ]
    for args in bad:
        with pytest.raises(ValueError) as want:
            utils.corr_pyramid(*args)
        for fn in (utils.corr_pyramid_fused, utils.CorrLookup.from_fmaps):
            with pytest.raises(ValueError) as got:
                fn(*args)
            assert str(got.value) == str(want.value)


# ---- 11 (host part). what the kernels do not take returns the mirror
@pytest.mark.parametrize('case', G23)
def test_cpu_and_fp64_lists_take_the_mirror_bit_for_bit(case):
    from motionpriorcmax_amd import utils
    g, f1, f2, nls, L = fixture(case)
    want, wtix = utils.corr_pyramid(f1, f2, nls)
    got, tix = utils.corr_pyramid_fused(f1, f2, nls)
    assert tix == wtix and all(torch.equal(x, y) and x.shape == y.shape for x, y in zip(got, want))
    got64, _ = utils.corr_pyramid_fused([t.double() for t in f1], [t.double() for t in f2], nls)
    assert all(x.dtype == torch.float64 and torch.equal(x, y.double()) for x, y in zip(got64, want))     # (the fixtures are exact in fp32)
    a = [t.clone().requires_grad_(True) for t in f1]
    levels, _ = utils.corr_pyramid_fused(a, f2, nls)
    ga = torch.autograd.grad(levels[-1].sum(), a, allow_unused=True)
    assert ga[1] is not None and torch.equal(ga[1], torch.autograd.grad(utils.corr_pyramid(a, f2, nls)[0][-1].sum(), a, allow_unused=True)[1])
