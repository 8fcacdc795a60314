"""The correlation lookup (csrc/corr_lookup.hip) element by element against the float64 reference of tests/corr_cases.py, through
utils.CorrLookup.lookup / lookup_bezier and their backward with every gradient: the first lookup of a forward (control points zero:
integer, half and quarter coordinates), a lattice of quarter coordinates through every clipping state of the window, fractions in
(-1, 0) down to the one that rounds to 1.0f, every radius at a grid below, at and past a chunk of 64 queries, 16 targets with 16
control points (ragged and full), one control point, six levels, NaN / inf / 1e30 / 2^20 coordinates and control points, and
operands that start one float into their buffers.

Every bound is the running error bound derived in tests/corr_cases.py from the roundings counted in the kernels; no element is
excused, and the figures are printed before they are asserted (pytest -s).  Beside the bounds: lookup_bezier is bit for bit
lookup at the replayed fp32 centres, the lane-per-query forward is bit for bit the default one, the accumulate route adds inside the
windows and leaves every other element bit for bit, and no launch writes outside its outputs or leaves an element of them unwritten
(guard bands and a NaN fill around buffers handed to the C entry points directly).

Measured on an MI355X (profiles/corr_cases_runs.md has every output): the largest error-to-bound ratios are 0.79 for the forward (the
tie that rounds a fraction to 1.0f; 0.73 elsewhere), 0.18 / 0.17 for grad_coords / grad_params, 0.50 for a grad_level cell on either
route.  53 tests in 4 s; under the bounds-checked build 0 violations."""
import ctypes

import pytest
import torch

import corr_cases as CK

pytestmark = pytest.mark.gpu

ONE_EACH = {'k_corr_lookup_fwd': 1, 'k_corr_lookup_bwd': 1}
GUARD = 64                                     # floats on either side of a guarded output (a multiple of 4: alignment is the view's own)
PATTERN = 0x7FC0BEEF                           # a NaN bit pattern
BOOK = {}                                      # output kind -> what CK.compare collects (printed by the last test)


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


def _put(t, offset):
    """On the device; `offset`: as a contiguous view that starts one float into a larger buffer."""
    if not offset:
        return t.to(_dev()).contiguous()
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _setup(name, level_grad=True):
    from motionpriorcmax_amd import utils
    cs = CK.case(name)
    levels = [_put(lv, cs.offset).requires_grad_(level_grad) for lv in cs.levels]
    return cs, utils.CorrLookup(levels, cs.nl, radius=cs.r)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _basis(cs, lk):
    bm = lk._basis(cs.times, cs.d, _dev(), torch.float32)
    assert _bits(bm.cpu(), cs.basis)               # the replay used the matrix the lookup uploads
    return bm


@pytest.mark.parametrize('name', CK.CASES)
def test_every_element_against_float64(name):
    from motionpriorcmax_amd import ops
    cs, lk = _setup(name)
    ref = CK.expected(name)
    go = _put(cs.g, cs.offset)
    c = _put(cs.coords, cs.offset).requires_grad_(True)
    assert lk._kernels_serve(c, 0)
    with ops.KernelTimer() as kt:
        out_c = lk.lookup(c)
        grads_c = torch.autograd.grad(out_c, [c] + lk.levels, go)
    assert _launches(kt) == ONE_EACH, _launches(kt)
    CK.compare_all(f'{name} coords', ref, out=out_c, gc=grads_c[0], gl=grads_c[1:], book=BOOK)
    produced = [out_c] + list(grads_c)
    if cs.params is not None:
        p = _put(cs.params, cs.offset).requires_grad_(True)
        assert lk._kernels_serve(p, cs.d)
        _basis(cs, lk)
        with ops.KernelTimer() as kt:
            out_b = lk.lookup_bezier(p, cs.times)
            grads_b = torch.autograd.grad(out_b, [p] + lk.levels, go)
        assert _launches(kt) == ONE_EACH, _launches(kt)
        CK.compare_all(f'{name} bezier', ref, out=out_b, gp=grads_b[0], gl=grads_b[1:], book=BOOK)
        # "the same expression per output": the Bezier mode is the coords mode at the centres corr_centre forms
        assert _bits(out_b, out_c), 'lookup_bezier(p) differs from lookup(replayed centres)'
        assert all(_bits(a, b) for a, b in zip(grads_b[1:], grads_c[1:]))
        produced += list(grads_b) + [out_b]
    assert all(bool(torch.isfinite(t).all()) for t in produced)


@pytest.mark.parametrize('name', CK.CASES)
def test_lane_per_query_forward_gives_the_same_bits(name):
    from motionpriorcmax_amd import ops, _lib as C
    cs, lk = _setup(name, level_grad=False)
    c = _put(cs.coords, cs.offset)
    p = _put(cs.params, cs.offset) if cs.params is not None else None
    want = [lk.lookup(c)] + ([lk.lookup_bezier(p, cs.times)] if p is not None else [])
    lk.flags = C.CORR_F_LANE_PER_QUERY
    with ops.KernelTimer() as kt:
        got = [lk.lookup(c)] + ([lk.lookup_bezier(p, cs.times)] if p is not None else [])
    assert _launches(kt) == {'k_corr_lookup_fwd_lane': len(got)}, _launches(kt)
    assert all(_bits(a, b) for a, b in zip(got, want))
    CK.compare(f'{name} lane per query', 'out', got[0], CK.expected(name).out, CK.expected(name).e_out, book=BOOK)


@pytest.mark.parametrize('name', CK.CASES)
def test_accumulate_route_adds_inside_the_windows_and_nowhere_else(name):
    """MPC_CORR_F_GRAD_ACCUM through ops._corr_lookup_bwd over buffers that hold random finite values."""
    from motionpriorcmax_amd import ops, _lib as C
    cs, lk = _setup(name, level_grad=False)
    ref = CK.expected(name)
    pf = CK.prefill(cs)
    go = _put(cs.g, cs.offset)
    c = _put(cs.coords, cs.offset)
    bufs = [_put(t, cs.offset) for t in pf]
    with ops.KernelTimer() as kt:
        gc = ops._corr_lookup_bwd(lk, 0, c, None, go, True, bufs, flags=C.CORR_F_GRAD_ACCUM)
    assert _launches(kt) == {'k_corr_lookup_bwd': 1}, _launches(kt)
    CK.compare(f'{name} coords accumulate', 'grad_coords', gc, ref.gc, ref.e_gc, book=BOOK)
    CK.compare_accum(f'{name} coords', ref, pf, bufs, book=BOOK)
    if cs.params is not None:
        p = _put(cs.params, cs.offset)
        again = [_put(t, cs.offset) for t in pf]
        gp = ops._corr_lookup_bwd(lk, cs.d, p, _basis(cs, lk), go, True, again, flags=C.CORR_F_GRAD_ACCUM)
        CK.compare(f'{name} bezier accumulate', 'grad_params', gp, ref.gp, ref.e_gp, book=BOOK)
        assert all(_bits(a, b) for a, b in zip(again, bufs))


def _guarded(shape, offset, inside=None):
    """-> (buffer of int32 PATTERN, float view of `shape` inside it, guard floats on either side); inside: a value to fill the view with."""
    n = 1
    for v in shape:
        n *= int(v)
    start = GUARD + (1 if offset else 0)
    buf = torch.full((n + 2 * GUARD + 1,), PATTERN, dtype=torch.int32, device=_dev())
    view = buf.view(torch.float32)[start:start + n].view(shape)
    if inside is not None:
        view.fill_(inside)
    return buf, view, start, n


def _assert_guarded(what, buf, view, start, n):
    assert not bool(torch.isnan(view).any()), f'{what}: an element of the output was not written'
    assert bool((buf[:start] == PATTERN).all()) and bool((buf[start + n:] == PATTERN).all()), f'{what}: written outside the output'


@pytest.mark.parametrize('accum', [False, True])
@pytest.mark.parametrize('name', CK.GUARD_CASES)
def test_launches_write_their_outputs_whole_and_nothing_else(name, accum):
    """out, grad_coords / grad_params and every grad_level[l] lie inside larger buffers of a NaN bit pattern and go to
    mpc_corr_lookup_fwd / _bwd directly: afterwards no element inside is NaN (the accumulate route starts from zeros: it writes
    window cells only), and every guard element holds the pattern bit for bit."""
    from motionpriorcmax_amd import ops, _lib as C
    cs, lk = _setup(name, level_grad=False)
    K2 = (2 * cs.r + 1) ** 2
    go = _put(cs.g, cs.offset)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())        # noqa: E731
    modes = [(0, _put(cs.coords, cs.offset), None)]
    if cs.params is not None:
        modes.append((cs.d, _put(cs.params, cs.offset), _basis(cs, lk)))
    for d, x, bm in modes:
        bez = bm is not None
        label = f'{name} {"bezier" if bez else "coords"}{" accumulate" if accum else ""}'
        if not accum:
            for flags in (0, C.CORR_F_LANE_PER_QUERY):
                desc = C.CorrDesc.from_buffer_copy(lk.descriptor(d))
                desc.flags = flags
                o = _guarded((cs.B, cs.E * K2, cs.h, cs.w), cs.offset)
                ops._call('mpc_corr_lookup_fwd', _dev(), ctypes.byref(desc), None if bez else ptr(x), ptr(x) if bez else None, ptr(bm), ptr(o[1]))
                _assert_guarded(f'{label} out (flags {flags})', *o)
                CK.compare(f'{label} guarded', 'out', o[1], CK.expected(name).out, CK.expected(name).e_out, book=BOOK)
        desc = C.CorrDesc.from_buffer_copy(lk.descriptor(d))
        desc.flags = C.CORR_F_GRAD_ACCUM if accum else 0
        gx = _guarded(x.shape, cs.offset)
        gls = [_guarded(lv.shape, cs.offset, inside=0.0 if accum else None) for lv in lk.levels]
        for l, gb in enumerate(gls):
            desc.grad_level[l] = gb[1].data_ptr()
        ops._call('mpc_corr_lookup_bwd', _dev(), ctypes.byref(desc), None if bez else ptr(x), ptr(x) if bez else None, ptr(bm), ptr(go),
                  None if bez else ptr(gx[1]), ptr(gx[1]) if bez else None)
        _assert_guarded(f'{label} grad_{"params" if bez else "coords"}', *gx)
        for l, gb in enumerate(gls):
            _assert_guarded(f'{label} grad_level_{l}', *gb)
        ref = CK.expected(name)
        CK.compare(f'{label} guarded', 'grad_params' if bez else 'grad_coords', gx[1], ref.gp if bez else ref.gc, ref.e_gp if bez else ref.e_gc, book=BOOK)
        if accum:
            CK.compare_accum(f'{label} guarded', ref, [torch.zeros_like(lv) for lv in cs.levels], [gb[1] for gb in gls], book=BOOK)
        else:
            CK.compare_all(f'{label} guarded', ref, gl=[gb[1] for gb in gls], book=BOOK)


def test_zz_largest_ratio_per_output():
    """Printed for profiles/corr_cases_runs.md (pytest -s); every ratio recorded by the tests above is at most 1."""
    for kind in sorted(BOOK):
        n, elements, ratio, label, emax, bmax = BOOK[kind]
        print(f'LARGEST {kind}: ratio {ratio:.3f}  case `{label}`  error {emax:.3e}  bound {bmax:.3e}  comparisons {n}  elements {elements}')
        assert ratio <= 1.0
