"""The gradient of a learned RAFT-spline basis matrix through the fused nodes (basis_grad='fused': ops.CurveTrajFn,
ops.CvxCurveTrajFn, ops.CorrLookupFn / CorrLookupSharedFn with csrc/curve_basis.hip behind their unchanged backward kernels) against
the g21_curves fixtures of the unmodified reference and against the plain-torch mirrors in float64.

Tolerances: the rules of tests/test_curve_types_host.py, nothing fixed in advance -- what the frozen route produces too (the
trajectories / the lookup's output, the gradients of the control points, the mask and the levels) must be torch.equal to the frozen
route's; grad_basis and the network's gradients per element max(4 * err_X, (2 + ceil(log2 N)) * 2^-24 * S), S the float64 sum of the
element's absolute addends and N their count (from the fixture; for the seeded cases computed here from the float64 mirror, with
err_X = |mirror_fp32 - mirror_fp64| and N = 2 * B * sites).  Every figure is printed before it is asserted (pytest -s)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_curve_types_host import (BasisTap, check_elementwise, check_head, check_lookup, curve_type_of, head_inputs, lookup_of,
                                   network_of, run_head, run_lookup)
from test_gpu_curve_types import HEAD_FUSED

pytestmark = pytest.mark.gpu

REDUCTION = {'k_curve_basis_part': 1, 'k_curve_basis_sum': 1}
LOOKUP_FUSED = {'k_corr_lookup_fwd': 1, 'k_corr_lookup_bwd': 1}


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


def _run_head_fused(g, plain, params_grad=True):
    """tests/test_curve_types_host.py: run_head with the network training and basis_grad='fused'."""
    from motionpriorcmax_amd import utils
    dev = _dev()
    p, m, times, tile, shape, scale = head_inputs(g, dev)
    if not params_grad:
        p = p.detach()
    net = network_of(g, dev)
    tap = BasisTap(net)
    if plain:
        h, w = p.shape[-2:]
        traj, pos = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), curve_type_of(g), net, scale=scale, basis_grad='fused')
        cot, leaves = torch.from_numpy(g['g_plain']).to(dev), [p]
    else:
        traj, pos = utils.trajectories_from_curves(p, times, tile, shape, curve_type_of(g), net, scale=scale, up_mask=m, basis_grad='fused')
        cot, leaves = torch.from_numpy(g['g']).to(dev), [p, m]
    if not params_grad:
        leaves = leaves[1:]
    traj.backward(cot, inputs=leaves + list(net.parameters()))
    tap.handle.remove()
    return dict(traj=traj, pos=pos, grad_params=p.grad if params_grad else None, grad_mask=None if plain else m.grad, grad_basis=tap.out.grad,
                grad_net=[q.grad for q in net.parameters()], net=net)


def _run_lookup_fused(g, shared, params_grad=True):
    """tests/test_curve_types_host.py: run_lookup with the network training and basis_grad='fused'."""
    dev = _dev()
    lk, p, times = lookup_of(g, dev, shared)
    p.requires_grad_(params_grad)
    net = network_of(g, dev)
    tap = BasisTap(net)
    out = lk.lookup_curves(p, times, 'LEARNED', net, basis_grad='fused')
    out.backward(torch.from_numpy(g['g']).to(dev), inputs=([p] if params_grad else []) + list(net.parameters()) + ([lv for lv in lk.levels] if shared else []))
    tap.handle.remove()
    return dict(out=out, grad_params=p.grad, grad_basis=tap.out.grad, grad_net=[q.grad for q in net.parameters()], net=net, lookup=lk)


@pytest.mark.parametrize('plain', [False, True])
@pytest.mark.parametrize('case', ['learned1', 'learned3', 'learned10', 'learned16'])
def test_head_fixtures_with_the_network_training(case, plain):
    """The launches of the frozen route plus the reduction's two kernels (and, with the mask, the rows kernel); the frozen route's
    bits for what it produces too; grad_basis and the network's gradients within the fixture's per-element bounds."""
    from motionpriorcmax_amd import ops
    g = load_golden('g21_curves_' + case)
    with ops.KernelTimer() as kt:
        res = _run_head_fused(g, plain)
    want = dict(HEAD_FUSED[plain], **REDUCTION)
    if not plain:
        want['k_pec_head_rows'] = 1
    assert _launches(kt) == want, _launches(kt)
    frozen = run_head(g, _dev(), plain=plain, frozen=True)
    assert torch.equal(res['traj'], frozen['traj']) and torch.equal(res['grad_params'], frozen['grad_params'])
    if not plain:
        assert torch.equal(res['grad_mask'], frozen['grad_mask'])
    assert res['grad_basis'].dtype == torch.float32 and res['grad_basis'].shape == g['grad_basis64'].shape
    check_head(case + ' (fused)', g, res, plain)


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('case', ['corr_a', 'corr_b', 'corr_c'])
def test_lookup_fixtures_with_the_network_training(case, shared):
    from motionpriorcmax_amd import ops
    g = load_golden('g21_curves_' + case)
    with ops.KernelTimer() as kt:
        res = _run_lookup_fused(g, shared)
    assert _launches(kt) == dict(LOOKUP_FUSED, **REDUCTION), _launches(kt)
    dev = _dev()
    lk, p, times = lookup_of(g, dev, shared)                # the frozen route, the level gradients included
    p.requires_grad_(True)
    net = network_of(g, dev).requires_grad_(False)
    out = lk.lookup_curves(p, times, 'LEARNED', net)
    out.backward(torch.from_numpy(g['g']).to(dev), inputs=[p] + (list(lk.levels) if shared else []))
    assert torch.equal(res['out'], out) and torch.equal(res['grad_params'], p.grad)
    if shared:
        for a, b in zip(res['lookup'].levels, lk.levels):
            assert a.grad is not None and torch.equal(a.grad, b.grad)
    assert res['grad_basis'].dtype == torch.float32
    check_lookup(case + ' (fused)', g, res)
    # params detached (detach_bezier): the backward launch writes the coordinate gradient alone; the same bits
    with ops.KernelTimer() as kt:
        det = _run_lookup_fused(g, shared, params_grad=False)
    assert _launches(kt) == dict(LOOKUP_FUSED, **REDUCTION), _launches(kt)
    assert det['grad_params'] is None and torch.equal(det['grad_basis'], res['grad_basis'])
    assert all(torch.equal(a, b) for a, b in zip(det['grad_net'], res['grad_net']))


# ---------------------------------------------------------------- order and determinism: sites = 2 * 64 + 7, two workgroups

SB, SD, ST, SH, SW = 2, 10, 5, 5, 27                        # B, d, T, grid: 135 sites a sample, 270 (sample, site) pairs
STILE, SSCALE = 8, 1.5                                    # (tile 8 on the 8h x 8w image: one centre per cell, 135 sites for both heads)
S_LEVELS, S_RADIUS, S_FEATURES = [2, 1, 2, 1, 1], 2, 8


class _Table(torch.nn.Module):
    """A 'basis network' whose output IS its parameter: the matrix [T, d] (the Jacobian is the identity)."""

    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(w.clone())

    def forward(self, t):
        return self.w + 0 * t


def _seeded(seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(params=torch.randn(SB, 2 * SD, SH, SW, generator=gen), mask=torch.randn(SB, 576, SH, SW, generator=gen),
                bm=torch.randn(ST, SD, generator=gen) * 0.5, times=[float(t) for t in torch.linspace(0.1, 0.9, ST)],
                fmap1=torch.randn(SB, S_FEATURES, SH, SW, generator=gen), fmap2=torch.randn(ST, SB, S_FEATURES, SH, SW, generator=gen), gen=gen)


def _lookup_params(s):
    """The rule of tests/test_gpu_curve_types.py: _polynomial_params for this learned matrix: the control points of every pixel
    where a centre / 2^l lies within 2^-9 of an integer are drawn again (at most 64 times); the margin 2^-10 is asserted."""
    from motionpriorcmax_amd import utils
    p, bm, nl = s['params'].clone() * 0.5, s['bm'].double(), max(S_LEVELS)

    def margin(q):
        c = utils.coords_grid(SB, SH, SW, 'cpu', torch.float64)[None] + torch.einsum('bcdhw,td->tbchw', q.double().reshape(SB, 2, SD, SH, SW), bm)
        return torch.stack([(c / 2 ** l - torch.round(c / 2 ** l)).abs() for l in range(nl)]).amin(dim=(0, 1, 3))        # [B, h, w]

    for _ in range(64):
        near = margin(p) < 2.0 ** -9
        if not bool(near.any()):
            break
        p = torch.where(near[:, None], torch.randn(p.shape, generator=s['gen']) * 0.5, p)
    assert float(margin(p).min()) >= 2.0 ** -10
    return p


def _mirror(node, s, p0, cot, dt):
    """The plain-torch mirror on CPU tensors of dtype dt -> (grad_basis, S): S[t][j] the sum of the absolute addends (float64 only)."""
    from motionpriorcmax_amd import utils
    from motionpriorcmax_amd.utils import basis as Bm, corr as corr_mod
    p, bm = p0.to(dt), s['bm'].to(dt).clone().requires_grad_(True)
    if node == 'lookup':
        levels, _ = utils.corr_pyramid(s['fmap1'].to(dt), s['fmap2'].to(dt), S_LEVELS)
        lk = utils.CorrLookup(levels, S_LEVELS, radius=S_RADIUS)
        coords = utils.coords_grid(SB, SH, SW, 'cpu', dt)[None] + torch.einsum('bcdhw,td->tbchw', p.reshape(SB, 2, SD, SH, SW), bm)
        coords.retain_grad()
        corr_mod._lookup_mirror(lk.levels, lk.target_indices, lk.radius, coords).backward(cot.to(dt))
        G, R, scale = coords.grad, p.reshape(SB, 2, SD, SH * SW), 1.0             # G [T, B, (x, y), h, w]
        G = G.reshape(ST, SB, 2, SH * SW)
    else:
        H, W = SH * STILE, SW * STILE
        if node == 'plain':
            traj, _ = Bm._curve_trajectories(p, bm, STILE, H, W, SSCALE)
            R = p.reshape(SB, 2, SD, SH * SW)
        else:
            m = s['mask'].to(dt)
            H, W = 8 * SH, 8 * SW
            traj, pos = Bm._cvx_curve_trajectories(p, m, bm, STILE, H, W, SSCALE)
            R = Bm._cvx_upsample(p, m)[:, :, pos[:, 0], pos[:, 1]].reshape(SB, 2, SD, -1)
        traj.backward(cot.to(dt))
        G, scale = cot.to(dt).flip(-1).permute(1, 0, 3, 2), SSCALE                 # [B, T, n, (y, x)] -> [T, B, (x, y), n]
    S = scale * torch.einsum('tbcn,bcjn->tj', G.abs(), R.abs()) if dt == torch.float64 else None
    return bm.grad.numpy().astype(np.float64), None if S is None else S.detach().numpy()


def _fused(node, s, p0, cot):
    from motionpriorcmax_amd import utils
    dev = _dev()
    net = _Table(s['bm']).to(dev)
    p = p0.to(dev).requires_grad_(True)
    if node == 'lookup':
        levels, _ = utils.corr_pyramid(s['fmap1'].to(dev), s['fmap2'].to(dev), S_LEVELS)
        lk = utils.CorrLookup([lv.contiguous() for lv in levels], S_LEVELS, radius=S_RADIUS)
        out = lk.lookup_curves(p, s['times'], 'LEARNED', net, basis_grad='fused')
    elif node == 'plain':
        out, _ = utils.trajectories_from_curves(p, s['times'], STILE, (SH * STILE, SW * STILE), 'LEARNED', net, scale=SSCALE, basis_grad='fused')
    else:
        out, _ = utils.trajectories_from_curves(p, s['times'], STILE, (8 * SH, 8 * SW), 'LEARNED', net, scale=SSCALE,
                                                up_mask=s['mask'].to(dev), basis_grad='fused')
    out.backward(cot.to(dev), inputs=[p, net.w])
    return net.w.grad


@pytest.mark.parametrize('node', ['plain', 'cvx', 'lookup'])
def test_the_sum_is_reproducible_and_within_the_bound_of_its_order(node):
    from motionpriorcmax_amd import ops
    s = _seeded(31)
    p0 = _lookup_params(s) if node == 'lookup' else s['params']
    if node == 'lookup':
        K, E = 2 * S_RADIUS + 1, sum(S_LEVELS)
        cot = torch.randn(SB, E * K * K, SH, SW, generator=s['gen'])
        sites = SH * SW
    else:
        sites = SH * SW if node == 'plain' else (8 * SH // STILE) * (8 * SW // STILE)
        cot = torch.randn(SB, ST, sites, 2, generator=s['gen'])
    assert sites == 2 * 64 + 7
    with ops.KernelTimer() as kt:
        a = _fused(node, s, p0, cot)
    assert all(_launches(kt).get(k) == 1 for k in REDUCTION), _launches(kt)
    b = _fused(node, s, p0, cot)
    assert torch.equal(a, b)
    m32, _ = _mirror(node, s, p0, cot, torch.float32)
    m64, S = _mirror(node, s, p0, cot, torch.float64)
    N = 2 * SB * sites
    bound = np.maximum(4.0 * np.abs(m32 - m64), (2 + math.ceil(math.log2(N))) * 2.0 ** -24 * S)
    check_elementwise(f'{node} grad_basis against the float64 mirror (N = {N})', a, m64, bound)


def test_bf16_control_points_and_mask_give_the_bits_of_the_upcast_tensors():
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_learned3')
    dev = _dev()
    p, m, times, tile, shape, scale = head_inputs(g, dev, grad=False)
    cot = torch.from_numpy(g['g']).to(dev)
    got = []
    for conv in (lambda t: t.bfloat16(), lambda t: t.bfloat16().float()):
        net = network_of(g, dev)
        tap = BasisTap(net)
        pp, mm = conv(p).requires_grad_(True), conv(m).requires_grad_(True)
        traj, _ = utils.trajectories_from_curves(pp, times, tile, shape, 'LEARNED', net, scale=scale, up_mask=mm, basis_grad='fused')
        traj.backward(cot, inputs=[pp, mm] + list(net.parameters()))
        tap.handle.remove()
        got.append((traj.detach(), tap.out.grad))
    assert got[0][1].dtype == torch.float32 and got[0][0].dtype == torch.float32
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


@pytest.mark.parametrize('node', ['plain', 'cvx', 'lookup', 'lookup_shared'])
def test_no_host_synchronisation(node):
    from motionpriorcmax_amd import utils
    dev = _dev()
    if node.startswith('lookup'):
        g = load_golden('g21_curves_corr_c')
        lk0, p, tl = lookup_of(g, dev, node == 'lookup_shared')
        p.requires_grad_(True)
        leaves, cot = [p] + (list(lk0.levels) if node == 'lookup_shared' else []), torch.from_numpy(g['g']).to(dev)
    else:
        g = load_golden('g21_curves_learned10')
        p, m, tl, tile, shape, scale = head_inputs(g, dev)
        h, w = p.shape[-2:]
        leaves, cot = ([p] if node == 'plain' else [p, m]), torch.from_numpy(g['g_plain' if node == 'plain' else 'g']).to(dev)
    net = network_of(g, dev)
    times = torch.tensor(tl, device=dev)

    def step():
        if node.startswith('lookup'):                # (a lookup object per step, as a training step builds one per pyramid: host work only)
            lk = utils.CorrLookup(lk0.levels, lk0.num_levels_per_target, radius=lk0.radius, shared_grad=lk0.shared_grad)
            out = lk.lookup_curves(p, times, 'LEARNED', net, basis_grad='fused')
        elif node == 'plain':
            out, _ = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), 'LEARNED', net, scale=scale, basis_grad='fused')
        else:
            out, _ = utils.trajectories_from_curves(p, times, tile, shape, 'LEARNED', net, scale=scale, up_mask=m, basis_grad='fused')
        return torch.autograd.grad(out, leaves + list(net.parameters()), cot)

    want = step()                                # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_beyond_the_limits_fused_is_the_mirror():
    """d = 17: nothing of the library is launched, and the call is the 'mirror' call (the forward bit for bit; the gradients, whose
    torch backward adds with atomics in the lookup, to 1e-5 of their largest element)."""
    from motionpriorcmax_amd import ops, utils
    dev, d, T = _dev(), 17, 3
    gen = torch.Generator().manual_seed(17)
    p0, w0 = torch.randn(1, 2 * d, 5, 7, generator=gen) * 0.3, torch.randn(T, d, generator=gen) * 0.5
    times, tile = [0.25, 0.5, 1.0], 4
    levels, _ = utils.corr_pyramid(torch.randn(1, 8, 5, 7, generator=gen).to(dev), torch.randn(T, 1, 8, 5, 7, generator=gen).to(dev), [2, 1, 1])
    res = {}
    for route in ('mirror', 'fused'):
        net, p = _Table(w0).to(dev), p0.to(dev).requires_grad_(True)
        lk = utils.CorrLookup([lv.contiguous() for lv in levels], [2, 1, 1], radius=2)
        with ops.KernelTimer() as kt:
            traj, _ = utils.trajectories_from_curves(p, times, tile, (5 * tile, 7 * tile), 'LEARNED', net, scale=2.0, basis_grad=route)
            out = lk.lookup_curves(p, times, 'LEARNED', net, basis_grad=route)
            grads = torch.autograd.grad([traj, out], [p, net.w], [torch.ones_like(traj), torch.ones_like(out)])
        assert _launches(kt) == {}, _launches(kt)
        res[route] = (traj.detach(), out.detach()) + grads
    a, b = res['mirror'], res['fused']
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max())
