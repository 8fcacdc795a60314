"""`utils.CorrLookup(..., shared_grad=True)` on the device: the lookups of one object add their level cotangents into one set of
buffers (ops.CorrGradGateFn / CorrLookupSharedFn; csrc/corr_lookup.hip: MPC_CORR_F_GRAD_ACCUM) instead of returning one volume-sized
gradient each.  Against the default path the comparison is torch.equal: both form a cell's cotangent by the same four-term sum and add
the iterations in the same order (the chain p_{k+1} = p_k + 0.01 * out_k forces N, N - 1, ..., 1), so only the sign of a zero may
differ.  Against float64 the rule of tests/test_corr_lookup_host.py holds: max |X_gpu - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|),
err_X the CPU fp32 mirror's error on the same sum, never taken from the kernel.  Figures are printed before they are asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_corr_lookup_host import assert_zero_where_fp64_is, check, maxdiff, redraw_to_margin

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 24, (1, 1, 1, 1, 4), 4, 10), (1, 8, 65, (3, 1), 3, 3)]       # (B, h, w, levels, radius, d)
D_FEAT = 8


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


@functools.lru_cache(maxsize=None)
def _data(shape):
    """CPU tensors, computed once per shape and never changed: feature maps, their pyramid, three parameter sets at the margin, the
    times and three output cotangents."""
    from motionpriorcmax_amd import utils
    B, h, w, nl, r, d = shape
    gen = torch.Generator().manual_seed(7100 + h)
    f1, f2 = torch.randn(B, D_FEAT, h, w, generator=gen), torch.randn(len(nl), B, D_FEAT, h, w, generator=gen)
    times = [(i + 1) / len(nl) for i in range(len(nl))]
    ps = [redraw_to_margin(torch.randn(B, 2 * d, h, w, generator=gen) * 3.0, times, max(nl), gen, 3.0) for _ in range(3)]
    levels, _ = utils.corr_pyramid(f1, f2, list(nl))
    K = 2 * r + 1
    gos = [torch.randn(B, sum(nl) * K * K, h, w, generator=gen) for _ in range(3)]
    return dict(f1=f1, f2=f2, times=times, ps=ps, levels=[lv.detach() for lv in levels], gos=gos)


def _lookup(shape, shared, device=None, dtype=torch.float32, level_grad=True):
    from motionpriorcmax_amd import utils
    device = device or _dev()
    lv = [t.detach().to(device, dtype).requires_grad_(level_grad) for t in _data(shape)['levels']]
    return utils.CorrLookup(lv, list(shape[3]), radius=shape[4], shared_grad=shared)


def _chain_loss(lk, x, times, gos, n, mode='bezier'):
    """n chained lookups on one object: x_{k+1} = x_k + 0.01 * (leading channels of out_k), loss = sum_k (out_k * go_k).sum()."""
    xk, loss, outs = x, 0.0, []
    for k in range(n):
        if mode == 'bezier':
            out = lk.lookup_bezier(xk, times)
            xk = xk + 0.01 * out[:, :x.shape[1]]
        else:
            out = lk.lookup(xk)
            T, B = x.shape[:2]
            xk = xk + 0.01 * out[:, :2 * T].reshape(B, T, 2, *x.shape[3:]).transpose(0, 1)
        outs.append(out)
        loss = loss + (out * gos[k % len(gos)]).sum()
    return loss, outs


def _centres(p, times):
    from test_corr_lookup_host import centres
    return centres(p, times)


def _equal(name, a, b):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape and torch.equal(a, b), (name, float((a - b).abs().max()))
    assert float(a.abs().max()) > 0, name


# ---- 1. the same values as the existing path

@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_a_chain_gives_the_gradients_of_the_default_path(shape, n):
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    res = []
    for shared in (False, True):
        lk = _lookup(shape, shared)
        assert (lk._token is not None) == shared
        p = z['ps'][0].to(_dev()).requires_grad_(True)
        loss, outs = _chain_loss(lk, p, z['times'], gos, n)
        res.append((outs, torch.autograd.grad(loss, [p] + lk.levels)))
        assert lk._gate is None or lk._gate.bufs is None
    for a, b in zip(res[0][0], res[1][0]):
        _equal('out', a, b)
    for i, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        _equal(f'grad {i}', a, b)


@pytest.mark.parametrize('shape', SHAPES)
def test_a_chain_of_lookup_coords_gives_the_gradients_of_the_default_path(shape):
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    res = []
    for shared in (False, True):
        lk = _lookup(shape, shared)
        c = _centres(z['ps'][0], z['times']).to(_dev()).requires_grad_(True)
        loss, _ = _chain_loss(lk, c, z['times'], gos, 3, mode='coords')
        res.append(torch.autograd.grad(loss, [c] + lk.levels))
    for i, (a, b) in enumerate(zip(*res)):
        _equal(f'grad {i}', a, b)


@pytest.mark.parametrize('shape', SHAPES)
def test_through_from_fmaps_the_feature_maps_get_the_same_gradients(shape):
    from motionpriorcmax_amd import ops, utils
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    res = []
    for shared in (False, True):
        f1, f2 = z['f1'].to(_dev()).requires_grad_(True), z['f2'].to(_dev()).requires_grad_(True)
        lk = utils.CorrLookup.from_fmaps(f1, f2, list(shape[3]), radius=shape[4], shared_grad=shared)
        assert (lk._token is not None) == shared and lk.levels[0].grad_fn is not None
        p = z['ps'][0].to(_dev()).requires_grad_(True)
        loss, _ = _chain_loss(lk, p, z['times'], gos, 3)
        with ops.KernelTimer() as kt:
            res.append(torch.autograd.grad(loss, [p, f1, f2]))
        assert _launches(kt)['k_corr_lookup_bwd'] == 3, _launches(kt)
    for name, a, b in zip(('grad_params', 'grad_fmap1', 'grad_fmap2'), *res):
        _equal(name, a, b)


# ---- 2. against float64

@pytest.mark.parametrize('shape', SHAPES)
def test_three_independent_lookups_against_float64(shape):
    z = _data(shape)
    nl = shape[3]

    def run(dtype, device, shared):
        lk = _lookup(shape, shared, device, dtype)
        ps = [p.detach().to(device, dtype).requires_grad_(True) for p in z['ps']]       # (detach: .to() may return the cached tensor itself)
        loss = sum((lk.lookup_bezier(p, z['times']) * go.to(device, dtype)).sum() for p, go in zip(ps, z['gos']))
        return torch.autograd.grad(loss, ps + lk.levels)

    m32, m64, got = run(torch.float32, 'cpu', False), run(torch.float64, 'cpu', False), run(torch.float32, _dev(), True)
    names = [f'grad_params_{k}' for k in range(3)] + [f'grad_level_{l}' for l in range(max(nl))]
    assert len(got) == len(names) and m64[0].dtype == torch.float64 and got[0].is_cuda
    for name, a32, a64, a in zip(names, m32, m64, got):
        a64 = a64.numpy()
        bound = max(4.0 * maxdiff(a32, a64), 2.0 ** -22 * float(np.abs(a64).max()))
        check(f'{shape[1]} x {shape[2]} {name}', maxdiff(a, a64), bound)
        if name.startswith('grad_level'):
            assert_zero_where_fp64_is(a, a64)


# ---- 3. the edges of the window

def _edge_coords(shape):
    """Centres far outside (-10, size + 10: the window lies wholly outside), straddling each border (partly outside) and inside, dealt
    over the pixels; level-0 coordinates, so the coarser levels see them at other offsets."""
    B, h, w, nl, r, d = shape
    gen = torch.Generator().manual_seed(33)
    T = len(nl)
    c = torch.rand(T, B, 2, h, w, generator=gen) * torch.tensor([w - 1.0, h - 1.0]).view(1, 1, 2, 1, 1)
    kind = torch.arange(h * w).view(h, w) % 10
    x, y = c[:, :, 0], c[:, :, 1]
    x[..., kind == 0] = -10.0
    x[..., kind == 1] = w + 10.0
    x[..., kind == 2] = -0.3
    x[..., kind == 3] = w - 0.6
    y[..., kind == 4] = -10.0
    y[..., kind == 5] = h + 10.0
    y[..., kind == 6] = -0.7
    y[..., kind == 7] = h - 0.4
    x[..., kind == 8] = -float(r) - 0.5                              # only the window's last column is inside
    y[..., kind == 8] = h + float(r) - 0.5                           # only its first row
    return c


@pytest.mark.parametrize('shape', SHAPES)
def test_windows_partly_and_wholly_outside_hit_three_times(shape):
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    res = []
    for shared in (False, True):
        lk = _lookup(shape, shared)
        c = _edge_coords(shape).to(_dev()).requires_grad_(True)
        loss = sum((lk.lookup(c) * go).sum() for go in gos)          # the same coordinates three times: the same cells three times
        res.append(torch.autograd.grad(loss, [c] + lk.levels))
    for i, (a, b) in enumerate(zip(*res)):
        _equal(f'grad {i}', a, b)
    wholly_outside = res[1][1].view(len(shape[3]), shape[0], shape[1] * shape[2], -1)[..., 0::10, :]       # pixels of kind 0: x = -10
    assert float(wholly_outside.abs().max()) == 0.0


# ---- 4. only what is asked

def test_the_parameters_alone_allocate_and_launch_nothing_for_the_levels():
    from motionpriorcmax_amd import ops
    shape = SHAPES[0]
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    lk = _lookup(shape, True)
    p = z['ps'][0].to(_dev()).requires_grad_(True)
    loss, _ = _chain_loss(lk, p, z['times'], gos, 3)
    level0_bytes = lk.levels[0].numel() * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with ops.KernelTimer() as kt:
        (gp,) = torch.autograd.grad(loss, [p], retain_graph=True)
    grew = torch.cuda.max_memory_allocated() - before
    print(f'backward to the parameters alone: peak memory grew by {grew} B; a grad_level_0 is {level0_bytes} B')
    assert _launches(kt) == {'k_corr_lookup_bwd': 3}, _launches(kt)
    assert lk._gate.bufs is None and grew < level0_bytes
    full = torch.autograd.grad(loss, [p] + lk.levels)
    assert torch.equal(full[0], gp) and lk._gate.bufs is None


def test_levels_without_requires_grad_get_no_gate():
    shape = SHAPES[1]
    z = _data(shape)
    p = z['ps'][0].to(_dev()).requires_grad_(True)
    res = []
    for shared in (False, True):
        lk = _lookup(shape, shared, level_grad=False)
        assert lk._gate is None and lk._token is None
        out = lk.lookup_bezier(p, z['times'])
        res.append((out, torch.autograd.grad(out, p, z['gos'][0].to(_dev()))[0]))
    _equal('out', res[0][0], res[1][0])
    _equal('grad_params', res[0][1], res[1][1])


# ---- 5. passes, 6. order

def test_two_passes_over_one_graph_and_the_order_of_the_nodes():
    shape = SHAPES[0]
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    lk = _lookup(shape, True)
    p = z['ps'][0].to(_dev()).requires_grad_(True)
    loss, outs = _chain_loss(lk, p, z['times'], gos, 3)
    events = []
    for k, out in enumerate(outs):
        out.grad_fn.register_hook(lambda gi, go, k=k: events.append(('lookup done', k, None if gi[-1] is None else 'tensor')))
    lk._token.grad_fn.register_prehook(lambda go: events.append(('gate starts', None if go[0] is None else 'tensor', lk._gate.bufs is not None)))
    want_order = [('lookup done', 2, None), ('lookup done', 1, None), ('lookup done', 0, None), ('gate starts', None, True)]
    a = torch.autograd.grad(loss, [p] + lk.levels, retain_graph=True)
    assert events == want_order, events              # the token's gradient is undefined, and the gate still runs last, with the buffers
    assert lk._gate.bufs is None
    b = torch.autograd.grad(loss, [p] + lk.levels, retain_graph=True)
    assert lk._gate.bufs is None
    for i, (x, y) in enumerate(zip(a, b)):
        _equal(f'second pass, grad {i}', x, y)
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a[1:], b[1:]))      # (a fresh set per pass)
    del events[:]
    loss.backward(retain_graph=True)
    assert events == want_order, events
    assert lk._gate.bufs is None
    for lv, g in zip(lk.levels, a[1:]):
        assert torch.equal(lv.grad, g)
    loss.backward()
    assert lk._gate.bufs is None
    for lv, g in zip(lk.levels, a[1:]):
        assert torch.equal(lv.grad, g + g)
    assert torch.equal(p.grad, a[0] + a[0])


# ---- 7. memory

def test_the_backward_pass_holds_one_level_set():
    """B = 1, 24 x 32, levels (1,1,1,1,4), leaf levels, 4 chained lookups: the rise of the allocated peak over the backward stays below
    1.5 level sets -- a condition from what the mode needs (one set, plus output-sized tensors of about a sixth of a set here), not a
    measurement.  Measured on an MI355X: 1.38 sets with the mode, 2.23 without (printed, not asserted)."""
    shape = (1, 24, 32, (1, 1, 1, 1, 4), 4, 10)
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    rise = {}
    for shared in (False, True):
        lk = _lookup(shape, shared)
        set_bytes = 4 * sum(lv.numel() for lv in lk.levels)
        p = z['ps'][0].to(_dev()).requires_grad_(True)
        loss, outs = _chain_loss(lk, p, z['times'], gos, 4)
        del outs
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        rise[shared] = torch.cuda.max_memory_allocated() - before
        assert all(lv.grad is not None for lv in lk.levels)
        del lk, p, loss
    print(f'peak rise over the backward of 4 chained lookups at 24 x 32: shared_grad=True {rise[True]} B = {rise[True] / set_bytes:.2f} level sets, '
          f'shared_grad=False {rise[False]} B = {rise[False] / set_bytes:.2f} level sets (a set is {set_bytes} B)')
    assert rise[True] < 1.5 * set_bytes, (rise, set_bytes)


# ---- 8. reproducibility

def _step(lk, p0, times, gos):
    p = p0.clone().requires_grad_(True)
    loss, outs = _chain_loss(lk, p, times, gos, 3)
    return (outs[-1].detach(),) + tuple(torch.autograd.grad(loss, [p] + lk.levels))


def test_two_runs_are_bitwise_equal_and_a_capture_replays_equal_to_eager():
    shape = SHAPES[0]
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    lk = _lookup(shape, True)
    args = (lk, z['ps'][0].to(_dev()), z['times'], gos)
    eager = [t.clone() for t in _step(*args)]
    again = _step(*args)
    assert len(eager) == len(again) == 2 + len(lk.levels)
    for a, b in zip(eager, again):
        _equal('second run', a, b)
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
    assert lk._gate.bufs is None
    for a, b in zip(static, eager):
        _equal('replay', a, b)


def test_no_host_synchronisation():
    shape = SHAPES[1]
    z = _data(shape)
    gos = [g.to(_dev()) for g in z['gos']]
    args = (_lookup(shape, True), z['ps'][0].to(_dev()), z['times'], gos)
    _step(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _step(*args)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out[1].shape == args[1].shape


# ---- 9. the ABI

@pytest.mark.parametrize('shape', SHAPES)
def test_the_flag_adds_to_window_cells_and_touches_nothing_else(shape):
    from motionpriorcmax_amd import ops, _lib as C
    z = _data(shape)
    B, h, w, nl, r, d = shape
    lk = _lookup(shape, False, level_grad=False)
    p, go = z['ps'][1].to(_dev()), z['gos'][1].to(_dev())
    basis = lk._basis(z['times'], d, _dev(), torch.float32).contiguous()
    gen = torch.Generator().manual_seed(5)
    pattern = [(torch.randn(lv.shape, generator=gen) + 3.0).to(_dev()) for lv in lk.levels]
    L = C.lib()

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(flags, bufs):
        desc = C.CorrDesc.from_buffer_copy(lk.descriptor(d))
        desc.flags = flags
        for l, t in enumerate(bufs):
            desc.grad_level[l] = None if t is None else t.data_ptr()
        gp = torch.full_like(p, float('nan'))
        with ops.KernelTimer() as kt:
            rc = L.mpc_corr_lookup_bwd(ctypes.byref(desc), None, ptr(p), ptr(basis), ptr(go), None, ptr(gp), None)
        torch.cuda.synchronize()
        assert rc == 0 and _launches(kt) == {'k_corr_lookup_bwd': 1}, (rc, _launches(kt))
        return gp

    fill = [torch.full_like(t, float('nan')) for t in pattern]
    gp_fill = call(0, fill)
    acc = [t.clone() for t in pattern]
    gp_acc = call(C.CORR_F_GRAD_ACCUM, acc)
    assert torch.equal(gp_acc, gp_fill) and torch.isfinite(gp_fill).all()
    K1 = 2 * r + 2
    for l, (a, f, pat) in enumerate(zip(acc, fill, pattern)):
        assert torch.isfinite(f).all()
        assert torch.equal(a, pat + f), l                         # outside the windows f is 0 and pat + 0 is pat: untouched
        changed = (a != pat).flatten(2).sum(dim=2)
        assert int(changed.max()) <= K1 * K1 and int(changed.sum()) > 0
    # one level only: the others are left as they are
    one = [t.clone() for t in pattern]
    call(C.CORR_F_GRAD_ACCUM, [None] + one[1:2] + [None] * (len(one) - 2))
    assert torch.equal(one[1], acc[1]) and all(torch.equal(a, b) for i, (a, b) in enumerate(zip(one, pattern)) if i != 1)
    # the flag with every grad_level NULL: as without the flag
    assert torch.equal(call(C.CORR_F_GRAD_ACCUM, [None] * len(pattern)), gp_fill)
