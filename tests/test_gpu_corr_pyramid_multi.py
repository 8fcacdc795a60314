"""The correlation pyramid over several references (events plus frames: utils.corr_pyramid_fused / CorrLookup.from_fmaps in list form,
ops.CorrPyramidMultiFn, csrc/corr_pyramid.hip) on the device.

  * the exact cases of tests/corr_pyramid_multi_cases.py: levels bit for bit, all 2R gradients bit for bit where sqrt(D) is a power of
    two and under the derived per-reference bound gamma(N + 8) * A elsewhere (D = 132); with levels left without a cotangent and with
    gradients asked for a subset of the 2R maps;
  * launch counts: the forward one k_corr_pyr_gemm and max_levels - 1 k_corr_pyr_pool whatever R is; the backward never more than
    the tensor form of the merged target list makes -- one gemm<2>, one reduce, one gemm<1>, one gather, the pools once;
  * the block-diagonal invariant: on randn inputs, levels (sliced by slot range) and all 2R gradients are torch.equal to the R
    tensor-form calls;
  * the g23 fixtures of the unmodified reference through CorrLookup.from_fmaps: levels and gradients bit for bit, lookup(coords) under
    the comparator and bounds of tests/corr_cases.py;
  * shared_grad=True over three chained lookup_bezier equals shared_grad=False; no host synchronisation; B = 0 launches nothing.

Measured on an MI355X: every level and every gradient at D in {4, 16, 64} bit for bit; the bounded gradients of `three_ragged`
(D = 132) at most 0.0049 of their bound (grad_fmap2 of reference 1); 24 tests in 3.5 s; under the bounds-checked build 0 violations."""
import types

import pytest
import torch

import corr_cases as CK
import corr_pyramid_multi_cases as MK
from test_corr_pyramid_multi_host import G23, MAPS, fixture

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


def _put(t, offset=False):
    """On the device; `offset`: as a contiguous view that starts 4 bytes off a 16-byte boundary."""
    if not offset:
        return t.to(_dev()).contiguous()
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _all(cs, value=True):
    return ((value,) * cs.R, (value,) * cs.R)


def _ref_levels(cs, r):
    return max(cs.nls[r])


def _expected_backward(cs, missing, want):
    """The launches of the backward: nothing per reference, and never more than the tensor form of the merged list."""
    w1, w2 = want
    have = lambda r, lo: any(l not in missing for l in range(lo, _ref_levels(cs, r)))          # noqa: E731
    out = {}
    gemm = int(any(w1)) + int(any(w2[r] and have(r, 0) for r in range(cs.R)))
    if gemm:
        out['k_corr_pyr_gemm'] = gemm
    if cs.L > 1 and any(w1[r] and have(r, 1) for r in range(cs.R)):
        out['k_corr_pyr_pool'] = cs.L - 1
    if any(w1[r] and MK.split_plan(cs, r, missing).S > 1 for r in range(cs.R)):
        out['k_corr_pyr_reduce'] = 1
    if any(w2):
        out['k_corr_pyr_gather'] = 1
    assert out.get('k_corr_pyr_gemm', 0) <= 2 and set(out) <= {'k_corr_pyr_gemm', 'k_corr_pyr_pool', 'k_corr_pyr_reduce', 'k_corr_pyr_gather'}
    return out


def _run(cs, missing=(), want=None, offset=False, inputs=None):
    """Forward and backward through utils.corr_pyramid_fused in list form -> (levels, g1 per reference, g2 per reference (None where
    not asked for), the launches of the forward, those of the backward)."""
    from motionpriorcmax_amd import ops, utils
    w1, w2 = want or _all(cs)
    f1, f2 = inputs or (cs.f1, cs.f2)
    a = [_put(t, offset).requires_grad_(w) for t, w in zip(f1, w1)]
    b = [_put(t, offset).requires_grad_(w) for t, w in zip(f2, w2)]
    cot = [_put(c, offset) for c in cs.cot]
    with ops.KernelTimer() as kf:
        levels, tix = utils.corr_pyramid_fused(a, b, cs.nls)
    assert tix == cs.tix and all(type(lv.grad_fn).__name__.startswith('CorrPyramidMultiFn') for lv in levels if any(w1 + w2))
    keep = [l for l in range(cs.L) if l not in missing]
    asked = [t for t in a + b if t.requires_grad]
    with ops.KernelTimer() as kb:
        grads = list(torch.autograd.grad([levels[l] for l in keep], asked, [cot[l] for l in keep])) if asked else []
    g1 = [grads.pop(0) if w else None for w in w1]
    g2 = [grads.pop(0) if w else None for w in w2]
    return [lv.detach() for lv in levels], g1, g2, _launches(kf), _launches(kb)


def _forward_launches(cs):
    return dict({'k_corr_pyr_gemm': 1}, **({'k_corr_pyr_pool': cs.L - 1} if cs.L > 1 else {}))


# ---- 6. the exact cases
@pytest.mark.parametrize('name', MK.CASES)
def test_every_element_of_the_exact_cases(name):
    cs = MK.case(name)
    levels, g1, g2, fwd, bwd = _run(cs, offset=(name == 'offset'))
    assert fwd == _forward_launches(cs), fwd
    assert bwd == _expected_backward(cs, (), _all(cs)), bwd
    for l, lv in enumerate(levels):
        assert lv.dtype == torch.float32 and lv.is_contiguous() and tuple(lv.shape) == (len(cs.tix[l]), cs.B * cs.hw, 1, cs.h >> l, cs.w >> l)
    for r in range(cs.R):
        assert g1[r].shape == cs.f1[r].shape and g2[r].shape == cs.f2[r].shape and g1[r].is_contiguous() and g2[r].is_contiguous()
    MK.compare_all(name, name, levels=levels, g1=g1, g2=g2)


# ---- 4. missing cotangents and partial gradients
@pytest.mark.parametrize('name', sorted(MK.MISSING))
def test_a_level_without_a_cotangent_is_a_missing_term(name):
    cs, missing = MK.case(name), MK.MISSING[name]
    levels, g1, g2, fwd, bwd = _run(cs, missing)
    assert fwd == _forward_launches(cs) and bwd == _expected_backward(cs, missing, _all(cs)), (fwd, bwd)
    MK.compare_all(f'{name} without {list(missing)}', name, missing, g1=g1, g2=g2)
    full = MK.expected(name)
    assert any(not torch.equal(g.cpu().double(), w.double()) for g, w in zip(g1 + g2, full.g1 + full.g2))


@pytest.mark.parametrize('name,want', [(n, w) for n in sorted(MK.PARTIAL) for w in MK.PARTIAL[n]])
def test_only_the_requested_gradients_are_computed(name, want):
    """A subset of the 2R maps requires grad: the others get None, the requested ones the bits they have beside all the others, and a
    reference none of whose maps requires grad adds no launch (the counts are those of the references that take part)."""
    cs = MK.case(name)
    _, all1, all2, _, _ = _run(cs)
    for missing in ((), MK.MISSING[name]):
        levels, g1, g2, fwd, bwd = _run(cs, missing, want)
        assert fwd == _forward_launches(cs) and bwd == _expected_backward(cs, missing, want), (want, missing, bwd)
        assert [g is not None for g in g1] == list(want[0]) and [g is not None for g in g2] == list(want[1])
        MK.compare_all(f'{name} {want} without {list(missing)}', name, missing, levels=levels, g1=g1, g2=g2)
        if not missing:
            assert all(torch.equal(g, w) for g, w in zip(g1 + g2, all1 + all2) if g is not None)


# ---- 7. the block-diagonal invariant
@pytest.mark.parametrize('name', ['base_model', 'three_ragged'])
def test_the_call_equals_the_tensor_form_calls_bit_for_bit(name):
    from motionpriorcmax_amd import utils
    cs = MK.case(name)
    gen = torch.Generator().manual_seed(71 + cs.D)
    f1 = [torch.randn(t.shape, generator=gen) for t in cs.f1]
    f2 = [torch.randn(t.shape, generator=gen) for t in cs.f2]
    rc = types.SimpleNamespace(**vars(cs))
    rc.cot = [torch.randn(c.shape, generator=gen) for c in cs.cot]
    for missing in ((), MK.MISSING[name]):
        levels, g1, g2, _, _ = _run(rc, missing, inputs=(f1, f2))
        for r in range(cs.R):
            a, b = _put(f1[r]).requires_grad_(True), _put(f2[r]).requires_grad_(True)
            alone, _ = utils.corr_pyramid_fused(a, b, cs.nls[r])
            assert all(type(lv.grad_fn).__name__.startswith('CorrPyramidFn') for lv in alone)
            keep = [l for l in range(len(alone)) if l not in missing]
            for l, lv in enumerate(alone):
                s0, n = MK.slots(cs, r, l)
                assert torch.equal(levels[l][s0:s0 + n], lv), (name, r, l)
            if keep:
                cots = [_put(rc.cot[l][MK.slots(cs, r, l)[0]:sum(MK.slots(cs, r, l))]) for l in keep]
                w1, w2 = torch.autograd.grad([alone[l] for l in keep], [a, b], cots)
            else:
                w1, w2 = torch.zeros_like(a), torch.zeros_like(b)
            assert torch.equal(g1[r], w1) and torch.equal(g2[r], w2), (name, r, missing)
            assert float(g1[r].abs().max()) > 0 or not keep


# ---- 8. the fixtures of the reference through the lookup
@pytest.mark.parametrize('case', G23)
def test_g23_through_the_lookup(case):
    from motionpriorcmax_amd import utils
    g, f1, f2, nls, L = fixture(case)
    a, b = [_put(t).requires_grad_(True) for t in f1], [_put(t).requires_grad_(True) for t in f2]
    lk = utils.CorrLookup.from_fmaps(a, b, nls, radius=int(g['radius']))
    assert all(type(lv.grad_fn).__name__.startswith('CorrPyramidMultiFn') for lv in lk.levels)
    assert lk.num_levels_per_target == nls[0] + nls[1]
    assert lk.target_indices == [[int(v) for v in g[f'target_indices_{l}']] for l in range(L)]
    for l, lv in enumerate(lk.levels):
        assert torch.equal(lv.detach().cpu(), torch.from_numpy(g[f'level_{l}'])), (case, l)
    coords = torch.from_numpy(g['coords'])
    out = lk.lookup(_put(coords))
    assert type(out.grad_fn).__name__.startswith('CorrLookup')
    # the comparator and the bounds of tests/corr_cases.py, over the fixture's levels and coordinates
    K = 2 * int(g['radius']) + 1
    ck = types.SimpleNamespace(coords=coords, levels=[torch.from_numpy(g[f'level_{l}']) for l in range(L)], r=int(g['radius']),
                               tix=lk.target_indices, params=None, g=torch.zeros(out.shape[0], lk.num_entries * K * K, *out.shape[2:]))
    ref = CK.reference(ck, want_levels=[False] * L)
    CK.compare(f'g23 {case}', 'out', out, ref.out, ref.e_out)
    # and against the reference's own fp32 output: the two distances to float64 together
    want = torch.from_numpy(g['out']).double()
    assert bool(((out.detach().cpu().double() - want).abs() <= ref.e_out + float(g['err_out'])).all())
    grads = torch.autograd.grad(lk.levels, a + b, [_put(torch.from_numpy(g[f'cot_{l}'])) for l in range(L)])
    for name, got in zip(MAPS, grads):
        assert torch.equal(got.cpu(), torch.from_numpy(g['grad_' + name])), (case, name)


# ---- 9. shared_grad on top of the merged pyramid
def test_shared_grad_over_three_chained_lookups_equals_the_plain_route():
    from motionpriorcmax_amd import ops, utils
    cs = MK.case('stops_at_0')
    d, r = 3, 2
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(cs.B, 2 * d, cs.h, cs.w, generator=gen)
    gos = [_put(torch.randn(cs.B, sum(cs.nl) * (2 * r + 1) ** 2, cs.h, cs.w, generator=gen)) for _ in range(3)]
    times = [(i + 1) / cs.T for i in range(cs.T)]
    results = []
    for shared in (False, True):
        a = [_put(t).requires_grad_(True) for t in cs.f1]
        b = [_put(t).requires_grad_(True) for t in cs.f2]
        params = _put(p0).requires_grad_(True)
        lk = utils.CorrLookup.from_fmaps(a, b, cs.nls, radius=r, shared_grad=shared)
        assert (lk._token is not None) == shared
        p, total = params, 0.0
        for k in range(3):                                                 # each lookup's output moves the next one's control points
            out = lk.lookup_bezier(p, times)
            total = total + (out * gos[k]).sum()
            p = p + 0.01 * out[:, :2 * d]
        with ops.KernelTimer() as kt:
            grads = torch.autograd.grad(total, a + b + [params])
        assert _launches(kt)['k_corr_lookup_bwd'] == 3, _launches(kt)
        results.append((grads, _launches(kt)))
    (plain, lp), (shared, ls) = results
    assert all(torch.equal(x, y) for x, y in zip(plain, shared))
    assert all(float(x.abs().max()) > 0 for x in shared)
    pyr = lambda d_: {k: v for k, v in d_.items() if k.startswith('k_corr_pyr')}          # noqa: E731
    assert pyr(lp) == pyr(ls) == _expected_backward(cs, (), _all(cs)), (lp, ls)


# ---- 10. no host synchronisation
def test_no_host_synchronisation():
    from motionpriorcmax_amd import utils
    cs = MK.case('stops_at_0')
    a, b = [_put(t).requires_grad_(True) for t in cs.f1], [_put(t).requires_grad_(True) for t in cs.f2]
    cot = [_put(c) for c in cs.cot]
    utils.corr_pyramid_fused(a, b, cs.nls)                                 # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        levels, _ = utils.corr_pyramid_fused(a, b, cs.nls)
        grads = torch.autograd.grad(levels, a + b, cot)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    MK.compare_all('no sync', 'stops_at_0', levels=levels, g1=grads[:cs.R], g2=grads[cs.R:])


# ---- 11. edge routing
def test_an_empty_batch_launches_nothing():
    from motionpriorcmax_amd import ops, utils
    a = [torch.zeros(0, 8, 6, 8, device=_dev(), requires_grad=True) for _ in range(2)]
    b = [torch.zeros(n, 0, 8, 6, 8, device=_dev(), requires_grad=True) for n in (2, 1)]
    with ops.KernelTimer() as kt:
        levels, tix = utils.corr_pyramid_fused(a, b, [[1, 2], [2]])
        grads = torch.autograd.grad([lv.sum() for lv in levels], a + b)
    assert _launches(kt) == {} and tix == [[0, 1, 2], [1, 2]]
    assert [tuple(lv.shape) for lv in levels] == [(3, 0, 1, 6, 8), (2, 0, 1, 3, 4)]
    assert all(g.shape == t.shape for g, t in zip(grads, a + b))


def test_what_the_kernels_do_not_take_returns_the_mirror():
    from motionpriorcmax_amd import ops, utils
    cs = MK.case('stops_at_0')
    want, _ = utils.corr_pyramid(cs.f1, cs.f2, cs.nls)
    a, b = [_put(t) for t in cs.f1], [_put(t) for t in cs.f2]
    for f1, f2 in (([t.double() for t in a], [t.double() for t in b]),                     # fp64
                   ([a[0], a[1].transpose(2, 3).contiguous().transpose(2, 3)], b)):        # a non-contiguous map
        with ops.KernelTimer() as kt:
            got, _ = utils.corr_pyramid_fused(f1, f2, cs.nls)
        assert _launches(kt) == {} and all(lv.grad_fn is None for lv in got)
        assert all(torch.equal(x.cpu().double(), y.double()) for x, y in zip(got, want))   # (integers: exact in either dtype)
    five = ([a[0]] * 5, [b[0][:1]] * 5, [[1]] * 5)                                         # more references than MPC_CORR_MAX_REFS
    with ops.KernelTimer() as kt:
        got, tix = utils.corr_pyramid_fused(*five)
    assert _launches(kt) == {} and tix == [[0, 1, 2, 3, 4]] and torch.equal(got[0][4], got[0][0])
