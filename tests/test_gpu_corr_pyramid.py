"""The fused RAFT-spline correlation pyramid on the device: utils.corr_pyramid_fused / CorrLookup.from_fmaps -> ops.CorrPyramidFn
(csrc/corr_pyramid.hip: mpc_corr_pyramid_fwd / _bwd).

Bitwise on the g16_corr fixtures of the unmodified reference (feature maps on a grid of 1/4, D in {4, 16}: every level and every
gradient is exact in fp32 whatever the summation order): the sha256 of each level against the fixture's, the gradients against float64
CPU autograd through utils.corr_pyramid (asserted representable in fp32 first).

Toleranced at the production k length and more than one tile, against utils.corr_pyramid in float64 on the CPU.  The bound is derived:
any-order fp32 summation of N products obeys |err| <= gamma * A, gamma = (N + 8) u / (1 - (N + 8) u), u = 2^-24; A is the same
expression in float64 on absolute values (float64 autograd through corr_pyramid on |fmap1|, |fmap2|, |cotangents|: every weight of
the chain is positive, so that is the backward formula on absolute values); N = D forward, the concatenated k length sum_l n_l h_l w_l
for grad_fmap1 and h * w (the products of one level's sum) for grad_fmap2; the 8 covers the scale, up to three pool steps of three
additions each and the level sum.  Every figure is printed before it is asserted (pytest -s shows them)."""
import hashlib

import pytest
import torch

from conftest import load_golden
from test_corr_lookup_host import CASES

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k: v['launches'] for k, v in kt.summary().items()}


def _fixture(case):
    g = load_golden('g16_corr_' + case)
    return g, torch.from_numpy(g['fmap1']), torch.from_numpy(g['fmap2']), [int(v) for v in g['num_levels']]


def _cotangents(levels, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.round(4.0 * torch.randn(lv.shape, generator=gen)) / 4.0 for lv in levels]


_REF = {}


def _reference(case):
    """(cotangents fp32 on the CPU, float64 CPU autograd gradients through utils.corr_pyramid for fmap1 and fmap2): computed once."""
    if case not in _REF:
        from motionpriorcmax_amd import utils
        g, f1, f2, nl = _fixture(case)
        a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
        levels, _ = utils.corr_pyramid(a, b, nl)
        cot = _cotangents(levels, 1600 + ord(case))
        g1, g2 = torch.autograd.grad(levels, [a, b], [c.double() for c in cot])
        for t in (g1, g2):
            assert torch.equal(t.float().double(), t), 'the float64 gradient is not representable in fp32'
        print(f'{case}: max |grad_fmap1| {float(g1.abs().max()):.4g}, max |grad_fmap2| {float(g2.abs().max()):.4g}')
        _REF[case] = (cot, g1.float(), g2.float())
    return _REF[case]


@pytest.mark.parametrize('case', CASES)
def test_forward_levels_are_the_references_bit_for_bit(case):
    from motionpriorcmax_amd import ops, utils
    g, f1, f2, nl = _fixture(case)
    with ops.KernelTimer() as kt:
        levels, tix = utils.corr_pyramid_fused(f1.to(_dev()), f2.to(_dev()), nl)
    assert _launches(kt) == dict(k_corr_pyr_gemm=1, **({'k_corr_pyr_pool': max(nl) - 1} if max(nl) > 1 else {})), _launches(kt)
    B, D, h, w = f1.shape
    assert len(levels) == max(nl) == len(tix)
    for l, lv in enumerate(levels):
        assert lv.is_cuda and lv.dtype == torch.float32 and lv.is_contiguous()
        assert tuple(lv.shape) == (len(tix[l]), B * h * w, 1, h >> l, w >> l)
        assert tix[l] == g[f'target_indices_{l}'].tolist() and all(isinstance(t, int) for t in tix[l])
        assert hashlib.sha256(lv.cpu().numpy().tobytes()).digest() == g[f'level_sha_{l}'].tobytes(), f'level {l}'


@pytest.mark.parametrize('case', CASES)
def test_backward_equals_float64_autograd_bit_for_bit(case):
    from motionpriorcmax_amd import utils
    g, f1, f2, nl = _fixture(case)
    cot, want1, want2 = _reference(case)
    dev = _dev()
    cot_d = [c.to(dev) for c in cot]

    def run(r1, r2, cots):
        a, b = f1.to(dev).requires_grad_(r1), f2.to(dev).requires_grad_(r2)
        levels, _ = utils.corr_pyramid_fused(a, b, nl)
        keep = [(lv, c) for lv, c in zip(levels, cots) if c is not None]
        return torch.autograd.grad([lv for lv, _ in keep], [t for t, r in ((a, r1), (b, r2)) if r], [c for _, c in keep])

    g1, g2 = run(True, True, cot_d)
    assert g1.dtype == torch.float32 and g1.shape == f1.shape and g2.shape == f2.shape and g1.is_contiguous() and g2.is_contiguous()
    assert torch.equal(g1.cpu(), want1) and torch.equal(g2.cpu(), want2)
    (only1,) = run(True, False, cot_d)
    (only2,) = run(False, True, cot_d)
    assert torch.equal(only1, g1) and torch.equal(only2, g2)
    # ---- one level's cotangent left unused (None): that level's term is missing from both gradients
    drop = len(cot) - 1
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    levels, _ = utils.corr_pyramid(a, b, nl)
    keep = [l for l in range(len(cot)) if l != drop]
    if keep:
        w1, w2 = torch.autograd.grad([levels[l] for l in keep], [a, b], [cot[l].double() for l in keep])
    else:
        w1, w2 = torch.zeros_like(a), torch.zeros_like(b)
    assert torch.equal(w1.float().double(), w1) and torch.equal(w2.float().double(), w2)
    n1, n2 = run(True, True, [c if l != drop else None for l, c in enumerate(cot_d)])
    assert torch.equal(n1.cpu(), w1.float()) and torch.equal(n2.cpu(), w2.float())


def _gamma(n):
    return (n + 8) * U / (1.0 - (n + 8) * U)


@pytest.mark.parametrize('shape', [(2, 256, 11, 13, (3, 1, 2)), (1, 20, 5, 7, (2,))])
def test_against_float64_at_the_derived_bound(shape):
    """B = 2, D = 256, 11 x 13, levels [3, 1, 2]: 143 positions = two tiles with a ragged edge in i and j, levels 11 x 13, 5 x 6, 2 x 3,
    the production k length.  D = 20, 5 x 7, [2]: a k tail that is no multiple of the k block."""
    from motionpriorcmax_amd import utils
    B, D, h, w, nl = shape
    nl = list(nl)
    gen = torch.Generator().manual_seed(256 + D)
    f1, f2 = torch.randn(B, D, h, w, generator=gen), torch.randn(len(nl), B, D, h, w, generator=gen)

    def run(a, b, cots, device, dtype):
        a, b = a.to(device, dtype).requires_grad_(True), b.to(device, dtype).requires_grad_(True)
        levels, tix = utils.corr_pyramid_fused(a, b, nl) if device != 'cpu' else utils.corr_pyramid(a, b, nl)
        if cots is None:
            return levels
        return [lv.detach() for lv in levels], torch.autograd.grad(levels, [a, b], [c.to(device, dtype) for c in cots])

    shapes = run(f1, f2, None, 'cpu', torch.float64)
    cots = [torch.randn(lv.shape, generator=gen) for lv in shapes]
    ref_l, (ref1, ref2) = run(f1, f2, cots, 'cpu', torch.float64)
    abs_l, (abs1, abs2) = run(f1.abs(), f2.abs(), [c.abs() for c in cots], 'cpu', torch.float64)
    got_l, (got1, got2) = run(f1, f2, cots, _dev(), torch.float32)
    tix = utils.level_target_indices(nl)
    kcat = sum(len(t) * (h >> l) * (w >> l) for l, t in enumerate(tix))
    assert kcat == {256: 3 * 143 + 2 * 30 + 6, 20: 35 + 6}[D]

    def bounded(label, got, ref, mag, n):
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == ref.shape
        err, bound = (got.cpu().double() - ref).abs(), _gamma(n) * mag
        worst = int(torch.argmax(err - bound))
        print(f'{label}: max |err| {float(err.max()):.4g}, smallest bound {float(bound.min()):.4g}, largest err / bound '
              f'{float((err / bound).max()):.4g} (err {float(err.flatten()[worst]):.4g}, bound {float(bound.flatten()[worst]):.4g})')
        assert bool((err <= bound).all()), label

    for l, (a, r, m) in enumerate(zip(got_l, ref_l, abs_l)):
        bounded(f'D {D} level {l}', a, r, m, D)
    bounded(f'D {D} grad_fmap1', got1, ref1, abs1, kcat)
    bounded(f'D {D} grad_fmap2', got2, ref2, abs2, h * w)


def _lookup_inputs(case):
    g, f1, f2, nl = _fixture(case)
    dev = _dev()
    return (f1.to(dev), f2.to(dev), nl, int(g['radius']), torch.from_numpy(g['params']).to(dev), [float(t) for t in g['times']],
            torch.from_numpy(g['g']).to(dev))


@pytest.mark.parametrize('case', ['a', 'c'])
def test_from_fmaps_looks_up_the_same_bits_as_the_existing_path(case):
    from motionpriorcmax_amd import utils
    f1, f2, nl, radius, p, times, _ = _lookup_inputs(case)
    lk = utils.CorrLookup.from_fmaps(f1, f2, nl, radius=radius)
    want = utils.CorrLookup(utils.corr_pyramid(f1, f2, nl)[0], nl, radius=radius)
    assert lk.radius == radius and lk.target_indices == want.target_indices
    assert torch.equal(lk.lookup_bezier(p, times), want.lookup_bezier(p, times))


@pytest.mark.parametrize('case', ['a', 'c'])
def test_the_chain_rule_through_lookup_and_pyramid(case):
    """One graph params / feature maps -> pyramid -> lookup, against the two nodes' backwards run one after the other by hand."""
    from motionpriorcmax_amd import ops, utils
    f1, f2, nl, radius, p, times, go = _lookup_inputs(case)
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    out = utils.CorrLookup.from_fmaps(a, b, nl, radius=radius).lookup_bezier(p, times)
    g1, g2 = torch.autograd.grad(out, [a, b], go)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all() and float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0
    levels, _ = utils.corr_pyramid_fused(f1, f2, nl)
    leaves = [lv.detach().requires_grad_(True) for lv in levels]
    gl = torch.autograd.grad(utils.CorrLookup(leaves, nl, radius=radius).lookup_bezier(p, times), leaves, go)
    a2, b2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    h1, h2 = torch.autograd.grad(ops.CorrPyramidFn.apply(a2, b2, nl), [a2, b2], gl)
    assert torch.equal(g1, h1) and torch.equal(g2, h2)


def _step(f1, f2, nl, cots):
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    from motionpriorcmax_amd import utils
    levels, _ = utils.corr_pyramid_fused(a, b, nl)
    return tuple(lv.detach() for lv in levels) + tuple(torch.autograd.grad(levels, [a, b], cots))


def _step_args(case='c'):
    _, f1, f2, nl = _fixture(case)
    cot, _, _ = _reference(case)
    return f1.to(_dev()), f2.to(_dev()), nl, [c.to(_dev()) for c in cot]


def test_no_host_synchronisation():
    args = _step_args()
    _step(*args)                                                 # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _step(*args)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out[-2].shape == args[0].shape and out[-1].shape == args[1].shape


def test_two_runs_are_bitwise_equal():
    args = _step_args()
    a, b = _step(*args), _step(*args)
    assert len(a) == len(b) == max(args[2]) + 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(x.abs().max()) > 0 for x in a)


def test_capture_replays_bitwise_equal_to_eager():
    """Forward + backward captured into a torch.cuda.graph on one stream and replayed (the pattern of test_gpu_corr_lookup.py)."""
    args = _step_args()
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
    assert len(static) == len(eager)
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


def test_an_empty_batch_launches_nothing():
    from motionpriorcmax_amd import ops, utils
    dev = _dev()
    f1 = torch.zeros(0, 16, 6, 8, device=dev, requires_grad=True)
    f2 = torch.zeros(2, 0, 16, 6, 8, device=dev, requires_grad=True)
    with ops.KernelTimer() as kt:
        levels, tix = utils.corr_pyramid_fused(f1, f2, [2, 1])
        g1, g2 = torch.autograd.grad([lv.sum() for lv in levels], [f1, f2])
    assert kt.summary() == {}
    assert tix == [[0, 1], [0]] and [tuple(lv.shape) for lv in levels] == [(2, 0, 1, 6, 8), (1, 0, 1, 3, 4)]
    assert all(lv.is_cuda and lv.grad_fn is not None and type(lv.grad_fn).__name__.startswith('CorrPyramidFn') for lv in levels)
    assert g1.shape == f1.shape and g2.shape == f2.shape
