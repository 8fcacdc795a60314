"""The RAFT-spline correlation lookup on the device: utils.CorrLookup.lookup / lookup_bezier -> ops.CorrLookupFn (csrc/corr_lookup.hip:
mpc_corr_lookup_fwd / _bwd) against the g16_corr fixtures of the unmodified reference (tools/gen_golden_corr.py) and, at two shapes
without a fixture, against the plain-torch mirror, at the tolerance rule of tests/test_corr_lookup_host.py: for every tensor
max |X_gpu - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|), err_X the fp32 error of the reference (fixture) or of the mirror on the
CPU -- never taken from the kernel.  Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_corr_lookup_host import CASES, assert_zero_where_fp64_is, centres, check, check_fixture, descriptor, lookup_of, maxdiff, redraw_to_margin

pytestmark = pytest.mark.gpu

ONE_EACH = {'k_corr_lookup_fwd': 1, 'k_corr_lookup_bwd': 1}


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


@pytest.mark.parametrize('case', CASES)
def test_goldens_through_the_public_functions(case):
    from motionpriorcmax_amd import ops
    g = load_golden('g16_corr_' + case)
    lk, p, times = lookup_of(g, _dev())
    assert lk._kernels_serve(p, p.shape[1] // 2)
    p.requires_grad_(True)
    go = torch.from_numpy(g['g']).to(_dev())
    with ops.KernelTimer() as kt:
        out = lk.lookup_bezier(p, times)
        grads = torch.autograd.grad(out, [p] + lk.levels, go)
    assert _launches(kt) == ONE_EACH, _launches(kt)
    c = centres(p.detach(), times).requires_grad_(True)
    with ops.KernelTimer() as kt:
        out_c = lk.lookup(c)
        (gc,) = torch.autograd.grad(out_c, c, go)
    assert _launches(kt) == ONE_EACH, _launches(kt)
    assert out.is_cuda and out_c.is_cuda and out_c.is_contiguous() and out_c.dtype == torch.float32
    assert gc.shape == c.shape and grads[0].shape == p.shape and all(a.shape == b.shape for a, b in zip(grads[1:], lk.levels))
    check_fixture(case, g, (out, grads[0], grads[1:], out_c, gc))


@pytest.mark.parametrize('case', ['b', 'c', 'd'])
def test_the_lane_per_query_forward_gives_the_same_bits(case):
    """MPC_CORR_F_LANE_PER_QUERY (the mapping that lost the probe's A/B, kept for it): the same expression per output, so the same bits."""
    from motionpriorcmax_amd import ops, _lib as C
    g = load_golden('g16_corr_' + case)
    lk, p, times = lookup_of(g, _dev(), level_grad=False)
    c = centres(p, times)
    want_b, want_c = lk.lookup_bezier(p, times), lk.lookup(c)
    lk.flags = C.CORR_F_LANE_PER_QUERY
    with ops.KernelTimer() as kt:
        got_b, got_c = lk.lookup_bezier(p, times), lk.lookup(c)
    assert _launches(kt) == {'k_corr_lookup_fwd_lane': 2}, _launches(kt)
    assert torch.equal(got_b, want_b) and torch.equal(got_c, want_c)
    check(f'{case} out (lane per query)', maxdiff(got_b, g['out64']), max(4.0 * float(g['err_out']), 2.0 ** -22 * float(np.abs(g['out64']).max())))


@pytest.mark.parametrize('shape', [(2, 16, 24, (1, 1, 1, 1, 4), 4, 10), (1, 8, 65, (3, 1), 3, 3)])
def test_against_the_mirror_where_there_is_no_fixture(shape):
    """The shipped level pattern on a 16 x 24 grid, and an 8 x 65 grid (a row one past a wave, three levels, radius 3).  err_X is the
    mirror in fp32 against the mirror in float64, both on the CPU, over the same fp32 pyramid."""
    from motionpriorcmax_amd import utils
    B, h, w, nl, r, d = shape
    gen = torch.Generator().manual_seed(1616 + h)
    f1, f2 = torch.randn(B, 4, h, w, generator=gen), torch.randn(len(nl), B, 4, h, w, generator=gen)
    times = [(i + 1) / len(nl) for i in range(len(nl))]
    p0 = redraw_to_margin(torch.randn(B, 2 * d, h, w, generator=gen) * 3.0, times, max(nl), gen, 3.0)
    levels, _ = utils.corr_pyramid(f1, f2, list(nl))
    K = 2 * r + 1
    go = torch.randn(B, sum(nl) * K * K, h, w, generator=gen)

    def run(dtype, device):
        lv = [t.detach().to(device, dtype).requires_grad_(True) for t in levels]
        lk = utils.CorrLookup(lv, list(nl), radius=r)
        p = p0.to(device, dtype).requires_grad_(True)
        out = lk.lookup_bezier(p, times)
        grads = torch.autograd.grad(out, [p] + lv, go.to(device, dtype))
        c = centres(p.detach(), times).requires_grad_(True)
        (gc,) = torch.autograd.grad(lk.lookup(c), c, go.to(device, dtype))
        return [out.detach(), grads[0], gc] + list(grads[1:])

    m32, m64, got = run(torch.float32, 'cpu'), run(torch.float64, 'cpu'), run(torch.float32, _dev())
    assert m64[0].dtype == torch.float64 and got[0].dtype == torch.float32 and got[0].is_cuda
    names = ['out', 'grad_params', 'grad_coords'] + [f'grad_level_{l}' for l in range(max(nl))]
    assert float((m64[0] == 0).double().mean()) < 0.9
    for name, a32, a64, a in zip(names, m32, m64, got):
        a64 = a64.numpy()
        bound = max(4.0 * maxdiff(a32, a64), 2.0 ** -22 * float(np.abs(a64).max()))
        check(f'{h} x {w} {name}', maxdiff(a, a64), bound)
        if name.startswith('grad_level'):
            assert_zero_where_fp64_is(a, a64)


def _case(name='c', level_grad=True):
    g = load_golden('g16_corr_' + name)
    lk, p, times = lookup_of(g, _dev(), level_grad=level_grad)
    return lk, p, times, torch.from_numpy(g['g']).to(_dev())


def _step(lk, p0, times, go):
    p = p0.clone().requires_grad_(True)
    out = lk.lookup_bezier(p, times)
    return (out.detach(),) + tuple(torch.autograd.grad(out, [p] + lk.levels, go))


def test_only_the_requested_gradients_are_produced():
    from motionpriorcmax_amd import ops
    lk, p, times, go = _case()
    full = _step(lk, p, times, go)
    c0 = centres(p, times)
    c = c0.clone().requires_grad_(True)
    (gc_full,) = torch.autograd.grad(lk.lookup(c), c, go)
    level0_bytes = lk.levels[0].numel() * 4
    # ---- coords alone: no level gradient is allocated
    frozen, _, _, _ = _case(level_grad=False)
    c = c0.clone().requires_grad_(True)
    out = frozen.lookup(c)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with ops.KernelTimer() as kt:
        (gc,) = torch.autograd.grad(out, c, go)
    grew = torch.cuda.max_memory_allocated() - before
    print(f'backward to coords alone: peak memory grew by {grew} B; a grad_level_0 is {level0_bytes} B')
    assert _launches(kt) == {'k_corr_lookup_bwd': 1} and grew < level0_bytes
    assert torch.equal(gc, gc_full)
    # ---- one level alone
    one, _, _, _ = _case(level_grad=False)
    one.levels[1].requires_grad_(True)
    out = one.lookup_bezier(p, times)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    (g1,) = torch.autograd.grad(out, one.levels[1], go)
    grew = torch.cuda.max_memory_allocated() - before
    print(f'backward to level 1 alone: peak memory grew by {grew} B')
    assert grew < level0_bytes and torch.equal(g1, full[3])
    # ---- none: under no_grad the forward allocates its output and nothing else
    with torch.no_grad():
        frozen.lookup_bezier(p, times)                          # (the cached basis of this object)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with ops.KernelTimer() as kt:
            out = frozen.lookup_bezier(p, times)
        peak = torch.cuda.max_memory_allocated() - before
    nbytes = out.numel() * 4
    print(f'forward under no_grad: peak memory grew by {peak} B; the output is {nbytes} B')
    assert _launches(kt) == {'k_corr_lookup_fwd': 1} and not out.requires_grad
    assert nbytes <= peak <= nbytes + 512 and torch.equal(out, full[0])


def test_two_runs_are_bitwise_equal():
    args = _case()
    a, b = _step(*args), _step(*args)
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(x.abs().max()) > 0 for x in a)


def test_capture_replays_bitwise_equal_to_eager():
    """Forward + backward captured into a torch.cuda.graph on one stream and replayed (the pattern of test_gpu_cvx_traj.py)."""
    args = _case()
    eager = [t.clone() for t in _step(*args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture
        for _ in range(2):
            _step(*args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(*args)
    graph.replay()
    torch.cuda.synchronize()
    assert len(static) == len(eager) == 4
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


def test_no_host_synchronisation_after_construction_with_the_level_list():
    args = _case()
    _step(*args)                                                 # warm-up: library load, the lookup's cached basis and descriptor
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _step(*args)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out[1].shape == args[1].shape and out[2].shape == args[0].levels[0].shape


def test_error_codes_come_back_through_the_abi_without_a_launch():
    from motionpriorcmax_amd import ops, _lib as C
    x = torch.zeros(1 << 16, device=_dev())
    v = ctypes.c_void_p(x.data_ptr())
    L = C.lib()

    def with_levels(desc):
        for l in range(min(desc.num_levels, C.CORR_MAX_LEVELS)):
            desc.level[l] = x.data_ptr()
        return ctypes.byref(desc)
    with ops.KernelTimer() as kt:
        for kw in (dict(radius=5), dict(d=17), dict(num_levels=[1] * 17), dict(h=256, w=256, num_levels=[7])):
            assert L.mpc_corr_lookup_fwd(with_levels(descriptor(**kw)), None, v, v, v, None) == C.E_UNSUPPORTED, kw
            assert L.mpc_corr_lookup_bwd(with_levels(descriptor(**kw)), None, v, v, v, None, v, None) == C.E_UNSUPPORTED, kw
        bad = descriptor()
        bad.level_h[2] = 13
        assert L.mpc_corr_lookup_fwd(with_levels(bad), v, None, None, v, None) == C.E_SHAPE
        assert L.mpc_corr_lookup_fwd(with_levels(descriptor(h=6, w=8, num_levels=[3])), v, None, None, v, None) == C.E_SHAPE
        assert L.mpc_corr_lookup_fwd(with_levels(descriptor()), v, v, v, v, None) == C.E_NULL           # coords AND params
        assert L.mpc_corr_lookup_fwd(with_levels(descriptor()), None, v, None, v, None) == C.E_NULL        # params without a basis
        assert L.mpc_corr_lookup_fwd(ctypes.byref(descriptor()), v, None, None, v, None) == C.E_NULL       # null levels
        assert L.mpc_corr_lookup_bwd(with_levels(descriptor()), v, None, None, v, None, v, None) == C.E_NULL   # grad_params in coords mode
        assert L.mpc_corr_lookup_fwd(with_levels(descriptor(B=0)), v, None, None, v, None) == 0            # B = 0 launches nothing
        assert L.mpc_corr_lookup_bwd(with_levels(descriptor(h=6, w=8, num_levels=[1], B=1)), v, None, None, v, None, None, None) == 0   # nothing asked for
    assert kt.summary() == {}
