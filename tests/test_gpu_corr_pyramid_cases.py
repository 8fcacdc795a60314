"""The correlation pyramid (csrc/corr_pyramid.hip) element by element against the exact references of tests/corr_pyramid_cases.py,
through utils.corr_pyramid_fused and its backward: the interior fast path of both loaders in all three products, vectorised ragged
tiles and 16-byte loads with a tail, the scalar loader, the split of both backward products up to its cap with uneven ranges,
more than one n tile above level 0, m tiles with a remainder beyond the first, D = 512, 16 targets over six levels down to 1 x 1,
missing cotangents, and operands that start one float into their buffers.

The inputs are integers for which every sum of every order is exact in fp32 (asserted by the case builder), so the levels and,
where sqrt(D) is a power of two, both gradients are compared bit for bit with float64; the gradients at D = 8, 132, 160, 512 under the
derived bound gamma(N + 8) * A of tests/test_gpu_corr_pyramid.py.  No element is excused.  Beside that: a gradient asked for alone
has the bits it has beside the other, k_corr_pyr_reduce is launched exactly when the plan splits grad_fmap1, no launch writes outside
its outputs or beyond the reported workspace or leaves an element unwritten (guard bands of a NaN pattern around buffers handed to the
C entry points directly), and two runs are bitwise equal.

Measured on an MI355X (profiles/corr_pyramid_cases_runs.md): every level of every case (the forward at D = 8, 132, 160, 512 against
the one correctly rounded division) and every gradient at D in {4, 16, 64, 256} bit for bit; the largest error-to-bound ratios of the
bounded gradients are 0.0027 (grad_fmap1, d512) and 0.0028 (grad_fmap2, d132).  23 tests in 3 s; under the bounds-checked build
0 violations."""
import ctypes

import pytest
import torch

import corr_pyramid_cases as PK

pytestmark = pytest.mark.gpu

GUARD = 64                                     # floats on either side of a guarded output (a multiple of 4: alignment is the view's own)
PATTERN = 0x7FC0BEEF                           # a NaN bit pattern
BOOK = {}                                      # output kind -> what PK.compare collects (printed by the last test)
OFFERED = {}                                   # output kind -> elements of the outputs handed to PK.compare, counted from the shapes


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _put(t, offset=False):
    """On the device; `offset`: as a contiguous view that starts one float into a larger buffer."""
    if not offset:
        return t.to(_dev()).contiguous()
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _offer(cs, levels=False, g1=False, g2=False):
    vol = sum(len(ts) * cs.B * cs.hw * cs.N[l] for l, ts in enumerate(cs.tix))
    for kind, n in (('levels', vol if levels else 0), ('grad_fmap1', cs.f1.numel() if g1 else 0), ('grad_fmap2', cs.f2.numel() if g2 else 0)):
        OFFERED[kind] = OFFERED.get(kind, 0) + n


def _expected_launches(cs, missing, want1=True, want2=True, forward=True):
    P = PK.plan(cs, missing)
    pooled = any(l not in missing for l in range(1, cs.L))
    want = {'k_corr_pyr_gemm': int(forward) + int(want1) + int(want2)}
    pools = (cs.L - 1) * (int(forward) + int(want1 and pooled))
    if pools:
        want['k_corr_pyr_pool'] = pools
    if want1 and P.S > 1:
        want['k_corr_pyr_reduce'] = 1
    if want2:
        want['k_corr_pyr_gather'] = 1
    return want


def _run(cs, missing=(), want1=True, want2=True):
    """Forward and backward through utils.corr_pyramid_fused -> (levels, grad_fmap1 or None, grad_fmap2 or None, launch counts)."""
    from motionpriorcmax_amd import ops, utils
    a, b = _put(cs.f1).requires_grad_(want1), _put(cs.f2).requires_grad_(want2)
    cot = [_put(c) for c in cs.cot]
    with ops.KernelTimer() as kt:
        levels, tix = utils.corr_pyramid_fused(a, b, cs.nl)
        assert tix == cs.tix and all(type(lv.grad_fn).__name__.startswith('CorrPyramidFn') for lv in levels)
        keep = [l for l in range(cs.L) if l not in missing]
        grads = torch.autograd.grad([levels[l] for l in keep], [t for t, r in ((a, want1), (b, want2)) if r], [cot[l] for l in keep])
    grads = list(grads)
    return [lv.detach() for lv in levels], grads.pop(0) if want1 else None, grads.pop(0) if want2 else None, _launches(kt)


@pytest.mark.parametrize('name', PK.CASES)
def test_every_element_against_float64(name):
    cs = PK.case(name)
    levels, g1, g2, launches = _run(cs)
    assert launches == _expected_launches(cs, ()), launches
    assert ('k_corr_pyr_reduce' in launches) == (cs.S > 1)
    for l, lv in enumerate(levels):
        assert lv.dtype == torch.float32 and lv.is_contiguous() and tuple(lv.shape) == (len(cs.tix[l]), cs.B * cs.hw, 1, cs.h >> l, cs.w >> l)
    assert g1.shape == cs.f1.shape and g2.shape == cs.f2.shape and g1.is_contiguous() and g2.is_contiguous()
    _offer(cs, True, True, True)
    PK.compare_all(name, name, levels=levels, g1=g1, g2=g2, book=BOOK)
    # a gradient asked for alone: the same bits, and only its own launches
    _, only1, none, launches = _run(cs, want2=False)
    assert none is None and _bits(only1, g1) and launches == _expected_launches(cs, (), want2=False), launches
    _, none, only2, launches = _run(cs, want1=False)
    assert none is None and _bits(only2, g2) and launches == _expected_launches(cs, (), want1=False), launches


@pytest.mark.parametrize('name', sorted(PK.MISSING))
def test_a_level_without_a_cotangent_is_a_missing_term(name):
    """mixed without level 1, wide_l1 with level 1 alone (one range: no reduce launch), six_levels without levels 0 and 3: bit for
    bit the float64 reference without those terms."""
    cs = PK.case(name)
    missing, S = PK.MISSING[name]
    levels, g1, g2, launches = _run(cs, missing)
    assert launches == _expected_launches(cs, missing), launches
    assert ('k_corr_pyr_reduce' in launches) == (S > 1)
    _offer(cs, False, True, True)
    PK.compare_all(f'{name} without {list(missing)}', name, missing, g1=g1, g2=g2, book=BOOK)
    full = PK.expected(name)
    assert not torch.equal(g1.cpu(), full.g1) and not torch.equal(g2.cpu(), full.g2)


def _guarded(shape, offset):
    """-> (buffer of int32 PATTERN, float view of `shape` inside it, guard floats on either side)."""
    n = 1
    for v in shape:
        n *= int(v)
    start = GUARD + (1 if offset else 0)
    buf = torch.full((n + 2 * GUARD + 1,), PATTERN, dtype=torch.int32, device=_dev())
    view = buf.view(torch.float32)[start:start + n].view(shape)
    assert view.data_ptr() % 16 == (4 if offset else 0)
    return buf, view, start, n


def _assert_guarded(what, buf, view, start, n, written=True):
    if written:
        assert not bool(torch.isnan(view).any()), f'{what}: an element of the output was not written'
    elif written is not None:                                            # (None: a workspace -- only what lies around it is held)
        assert bool((buf[start:start + n] == PATTERN).all()), f'{what}: written by a call that had to launch nothing'
    assert bool((buf[:start] == PATTERN).all()) and bool((buf[start + n:] == PATTERN).all()), f'{what}: written outside the output'


def _direct(cs, offset, missing=(), ws_shift=0):
    """mpc_corr_pyramid_fwd and _bwd over guarded outputs and a workspace of exactly the reported size with a guard after it ->
    (levels, g1, g2 as guarded tuples, the two workspaces as guarded tuples, launches, return codes)."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    f1, f2, cot = _put(cs.f1, offset), _put(cs.f2, offset), [_put(c, offset) for c in cs.cot]
    desc, _ = ops.corr_pyramid_desc(cs.B, cs.h, cs.w, cs.nl)
    lv = [_guarded(c.shape, offset) for c in cs.cot]
    g1, g2 = _guarded(cs.f1.shape, offset), _guarded(cs.f2.shape, offset)
    for l in range(cs.L):
        desc.level[l] = lv[l][1].data_ptr()
        desc.grad_level[l] = None if l in missing else cot[l].data_ptr()
    P = PK.plan(cs)
    nbytes = [ops._query('mpc_corr_pyramid_workspace_bytes', dev, ctypes.byref(desc), cs.D, back) for back in (0, 1)]
    assert nbytes == [max(16, 4 * P.pooled), 4 * P.total_bwd]
    ws = [_guarded((nb // 4,), False) for nb in nbytes]                   # (the workspace stays 16-byte aligned)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() + ws_shift)             # noqa: E731
    with ops.KernelTimer() as kt:
        rc0 = ops._call('mpc_corr_pyramid_fwd', dev, ctypes.byref(desc), cs.D, ops._ptr(f1), ops._ptr(f2), ptr(ws[0][1]), accept=(C.E_NULL,))
        rc1 = ops._call('mpc_corr_pyramid_bwd', dev, ctypes.byref(desc), cs.D, ops._ptr(f1), ops._ptr(f2), ops._ptr(g1[1]), ops._ptr(g2[1]),
                        ptr(ws[1][1]), accept=(C.E_NULL,))
    return lv, g1, g2, ws, _launches(kt), (rc0, rc1)


@pytest.mark.parametrize('name,offset', [(n, False) for n in PK.GUARD_CASES] + [('offset', True)])
def test_launches_write_their_outputs_whole_and_nothing_else(name, offset):
    """The levels, grad_fmap1 and grad_fmap2 lie inside larger buffers of a NaN bit pattern, the workspace is a view of exactly the
    reported byte count with the pattern after it: afterwards no element inside an output is NaN, every guard element holds the
    pattern bit for bit, and the results are those of the ops path.  offset: fmap1, fmap2, every level, every cotangent and both
    gradients start one float into their buffers (4-byte aligned only: the scalar loaders and k_corr_pyr_gather<1> at w % 4 == 0)."""
    cs = PK.case(name)
    lv, g1, g2, ws, launches, rcs = _direct(cs, offset)
    assert rcs == (0, 0) and launches == _expected_launches(cs, ()), (rcs, launches)
    label = f'{name} guarded{" offset" if offset else ""}'
    for l, t in enumerate(lv):
        _assert_guarded(f'{label} level_{l}', *t)
    _assert_guarded(f'{label} grad_fmap1', *g1)
    _assert_guarded(f'{label} grad_fmap2', *g2)
    for back, t in enumerate(ws):
        _assert_guarded(f'{label} workspace (backward {back})', *t, written=None)
    _offer(cs, True, True, True)
    PK.compare_all(label, name, levels=[t[1] for t in lv], g1=g1[1], g2=g2[1], book=BOOK)
    levels, w1, w2, _ = _run(cs)
    assert all(_bits(a[1], b) for a, b in zip(lv, levels)) and _bits(g1[1], w1) and _bits(g2[1], w2)


def test_a_missing_cotangent_behind_guard_bands():
    cs = PK.case('six_levels')
    missing, _ = PK.MISSING['six_levels']
    lv, g1, g2, ws, launches, rcs = _direct(cs, False, missing)
    assert rcs == (0, 0) and launches == _expected_launches(cs, missing), (rcs, launches)
    for what, t in (('grad_fmap1', g1), ('grad_fmap2', g2)):
        _assert_guarded(f'six_levels without {list(missing)} {what}', *t)
    _assert_guarded('workspace', *ws[1], written=None)
    _offer(cs, False, True, True)
    PK.compare_all(f'six_levels guarded without {list(missing)}', 'six_levels', missing, g1=g1[1], g2=g2[1], book=BOOK)


def test_a_workspace_that_is_not_16_byte_aligned_is_refused_and_nothing_is_launched():
    from motionpriorcmax_amd import _lib as C
    cs = PK.case('offset')
    lv, g1, g2, ws, launches, rcs = _direct(cs, False, ws_shift=4)
    assert rcs == (C.E_NULL, C.E_NULL) and launches == {}, (rcs, launches)
    assert b'16-byte aligned' in C.lib().mpc_last_error_string()
    for t in lv + [g1, g2] + ws:
        _assert_guarded('refused call', *t, written=False)


@pytest.mark.parametrize('name', PK.REPEAT_CASES)
def test_two_runs_are_bitwise_equal(name):
    cs = PK.case(name)
    a, b = _run(cs), _run(cs)
    assert all(_bits(x, y) for x, y in zip(a[0], b[0])) and _bits(a[1], b[1]) and _bits(a[2], b[2])
    assert all(float(x.abs().max()) > 0 for x in a[0] + [a[1], a[2]])


def test_zz_summary_per_output():
    """Printed for profiles/corr_pyramid_cases_runs.md (pytest -s): per output the comparisons, the elements compared and how many of
    them bit for bit, the largest error-to-bound ratio of the bounded ones.  No element of any output is excluded."""
    assert set(BOOK) == set(k for k, v in OFFERED.items() if v)
    for kind in sorted(BOOK):
        n, elements, bitwise, ratio, label = BOOK[kind]
        excluded = 1.0 - elements / OFFERED[kind]
        print(f'SUMMARY {kind}: comparisons {n}  elements {elements}  bit for bit {bitwise}  bounded {elements - bitwise}  '
              f'largest error / bound {ratio:.4f} (`{label}`)  share excluded {excluded:.1f}')
        assert excluded == 0 and elements == OFFERED[kind] and ratio <= 1.0
        assert kind != 'levels' or bitwise == elements
