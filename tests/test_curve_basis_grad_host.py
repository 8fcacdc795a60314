"""The keyword basis_grad of utils.trajectories_from_curves and CorrLookup.lookup_curves, and the host side of mpc_curve_basis_grad,
without a GPU: the keyword is validated before anything else, 'mirror' is the call without the keyword bit for bit, 'fused' changes
nothing for CPU tensors (they take the plain-torch mirrors whatever it says), and the size query answers the limits of the nodes
without a device."""
import pytest
import torch

from conftest import load_golden
from test_curve_types_host import BasisTap, curve_type_of, head_inputs, lookup_of, network_of


def _head(g, plain, **kw):
    from motionpriorcmax_amd import utils
    p, m, times, tile, shape, scale = head_inputs(g)
    net = network_of(g)
    tap = BasisTap(net)
    if plain:
        h, w = p.shape[-2:]
        traj, _ = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), curve_type_of(g), net, scale=scale, **kw)
        cot, leaves = torch.from_numpy(g['g_plain']), [p]
    else:
        traj, _ = utils.trajectories_from_curves(p, times, tile, shape, curve_type_of(g), net, scale=scale, up_mask=m, **kw)
        cot, leaves = torch.from_numpy(g['g']), [p, m]
    grads = torch.autograd.grad(traj, leaves + [tap.out] + list(net.parameters()), cot)
    tap.handle.remove()
    return (traj.detach(),) + grads


def _lookup(g, **kw):
    lk, p, times = lookup_of(g)
    p.requires_grad_(True)
    net = network_of(g)
    tap = BasisTap(net)
    out = lk.lookup_curves(p, times, 'LEARNED', net, **kw)
    grads = torch.autograd.grad(out, [p, tap.out] + list(net.parameters()), torch.from_numpy(g['g']))
    tap.handle.remove()
    return (out.detach(),) + grads


@pytest.mark.parametrize('bad', ['FUSED', 'kernel', '', None, True])
def test_the_keyword_is_validated(bad):
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_learned3')
    p, m, times, tile, shape, scale = head_inputs(g, grad=False)
    net = network_of(g)
    with pytest.raises(ValueError, match='basis_grad'):
        utils.trajectories_from_curves(p, times, tile, shape, 'LEARNED', net, scale=scale, up_mask=m, basis_grad=bad)
    with pytest.raises(ValueError, match='basis_grad'):
        utils.trajectories_from_curves(p, times, tile, shape, 'BEZIER', up_mask=m, basis_grad=bad)        # (also where it would change nothing)
    gc = load_golden('g21_curves_corr_a')
    lk, pc, tl = lookup_of(gc)
    with pytest.raises(ValueError, match='basis_grad'):
        lk.lookup_curves(pc, tl, 'LEARNED', network_of(gc), basis_grad=bad)


@pytest.mark.parametrize('plain', [False, True])
def test_mirror_is_the_call_without_the_keyword_and_cpu_tensors_ignore_fused(plain):
    g = load_golden('g21_curves_learned3')
    want = _head(g, plain)
    for route in ('mirror', 'fused'):
        got = _head(g, plain, basis_grad=route)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), route


def test_lookup_mirror_is_the_call_without_the_keyword_and_cpu_tensors_ignore_fused():
    g = load_golden('g21_curves_corr_a')
    want = _lookup(g)
    for route in ('mirror', 'fused'):
        got = _lookup(g, basis_grad=route)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), route


def test_the_size_query_and_the_limits_are_host_only():
    from motionpriorcmax_amd import _lib as C
    L = C.lib()
    q = L.mpc_curve_basis_grad_scratch_floats
    assert q(6, 10, 13, 48 * 64) == 72 * 13 * 10             # ceil(6 * 3072 / 256) partials of [T][d]
    assert q(2, 10, 5, 135) == 2 * 5 * 10 and q(1, 16, 8, 256) == 8 * 16 and q(1, 1, 1, 257) == 2
    assert q(0, 10, 5, 135) == 0 and q(3, 10, 5, 0) == 0
    assert q(1, 17, 5, 135) == C.E_UNSUPPORTED and q(1, 16, 769, 135) == C.E_UNSUPPORTED and q(1, 16, 768, 135) > 0
    assert q(1, 0, 5, 135) == C.E_SHAPE and q(-1, 10, 5, 135) == C.E_SHAPE and q(1, 10, 0, 135) == C.E_SHAPE
    f = L.mpc_curve_basis_grad
    assert f(None, None, C.CBG_PLAIN, 1.0, None, None, 1, 17, 5, 135, None) == C.E_UNSUPPORTED        # (the limits come first: no launch)
    assert f(None, None, 3, 1.0, None, None, 1, 10, 5, 135, None) == C.E_UNSUPPORTED
    assert f(None, None, C.CBG_ROWS, 1.0, None, None, 1, 10, 5, 135, None) == C.E_NULL
    assert b'mpc_curve_basis_grad' in L.mpc_last_error_string()
