"""The reference's curve types POLYNOMIAL and LEARNED on the device: utils.trajectories_from_curves / flows_from_curves,
CorrLookup.lookup_curves and trajectory_val_metrics(curve_type=...) against the g21_curves fixtures of the unmodified reference
(tools/gen_golden_curves.py).  A basis matrix that is a constant to autograd (POLYNOMIAL; LEARNED with a frozen network or under
no_grad) runs in the fused nodes with exactly the launches of the Bezier functions; a basis network that trains takes the
plain-torch mirrors on the device (the fused nodes have no gradient for the matrix).

Tolerances: the helpers and rules of tests/test_curve_types_host.py -- max |X_gpu - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|) for
every tensor the Bezier nodes produce too, and per element max(4 * err_X, (2 + ceil(log2 N)) * 2^-24 * S) for grad_basis and the
network's gradients (S the float64 sum of the absolute addends, N their count).
Every figure is printed before it is asserted (pytest -s shows them)."""
import pytest
import torch

import val_metrics_oracle as O
from conftest import load_golden
from test_curve_types_host import (CORR_CASES, HEAD_CASES, check, check_head, check_lookup, curve_type_of, head_inputs,
                                   lookup_of, maxdiff, network_of, run_head, run_lookup, tol)

pytestmark = pytest.mark.gpu

HEAD_FUSED = {False: {'k_cvx_traj_fwd': 1, 'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1}, True: {'k_curve_traj_fwd': 1, 'k_curve_traj_bwd': 1}}


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


def _grads_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('plain', [False, True])
@pytest.mark.parametrize('case', HEAD_CASES)
def test_head_fixtures_through_the_public_functions(case, plain):
    """A constant basis: the Bezier launch set, every tensor within its bound, what the reference leaves exactly zero stays zero
    (check_head).  A learned basis that trains: no launch of the library (the mirror), every gradient within its bound; with the
    network frozen: the fused nodes again."""
    from motionpriorcmax_amd import ops, utils
    g = load_golden('g21_curves_' + case)
    learned = curve_type_of(g) == 'LEARNED'
    with ops.KernelTimer() as kt:
        res = run_head(g, _dev(), plain=plain)
    assert _launches(kt) == ({} if learned else HEAD_FUSED[plain]), _launches(kt)
    assert res['traj'].is_cuda
    check_head(case, g, res, plain)
    if learned:
        with ops.KernelTimer() as kt:
            res = run_head(g, _dev(), plain=plain, frozen=True)
        assert _launches(kt) == HEAD_FUSED[plain], _launches(kt)
        check_head(case + ' (frozen)', g, res, plain)
    if not plain:
        p, m, times, tile, shape, scale = head_inputs(g, _dev(), grad=False)
        with ops.KernelTimer() as kt, torch.no_grad():
            flows = utils.flows_from_curves(p, times, curve_type_of(g), network_of(g, _dev()), up_mask=m, scale=scale)
        assert _launches(kt) == {'k_cvx_flow_fwd': 1}, _launches(kt)
        check(f'{case} flows', maxdiff(flows[torch.from_numpy(g['flow_times']).to(_dev())], g['flows64']), tol(g, 'flows'))


@pytest.mark.parametrize('case', CORR_CASES)
@pytest.mark.parametrize('shared', [False, True])
def test_lookup_fixtures_through_the_public_functions(case, shared):
    from motionpriorcmax_amd import ops, utils
    g = load_golden('g21_curves_' + case)
    with ops.KernelTimer() as kt:
        res = run_lookup(g, _dev(), shared_grad=shared)
    assert _launches(kt) == {}, _launches(kt)                   # a basis network that trains: the mirror
    check_lookup(case, g, res)
    with ops.KernelTimer() as kt:
        res = run_lookup(g, _dev(), shared_grad=shared, frozen=True)
    assert _launches(kt) == {'k_corr_lookup_fwd': 1, 'k_corr_lookup_bwd': 1}, _launches(kt)
    check_lookup(case + ' (frozen)', g, res)
    _polynomial_lookup_against_the_mirror(case, g, shared)


def _polynomial_params(g, times, num_levels):
    """The fixture's control points, those of every pixel where a POLYNOMIAL centre / 2^l lies within 2^-10 of an integer drawn
    again (seeded; the rule of tools/gen_golden_curves.py: the coordinate gradient has a kink at integers and an fp32 coordinate is
    about 1e-6 off).  The margin is asserted."""
    from motionpriorcmax_amd import utils
    p = torch.from_numpy(g['params']).clone()
    B, _, h, w = p.shape
    amp, gen = float(p.abs().max()) / 3.0, torch.Generator().manual_seed(21)

    def centres(q):
        return utils.coords_grid(B, h, w, 'cpu', torch.float64)[None] + utils.flows_from_curves(q.double(), times, 'POLYNOMIAL')

    def margin(q):
        c = centres(q)
        return torch.stack([(c / 2 ** l - torch.round(c / 2 ** l)).abs() for l in range(num_levels)]).amin(dim=(0, 1, 3))    # [B, h, w]

    for _ in range(64):
        near = margin(p) < 2.0 ** -9
        if not bool(near.any()):
            break
        p = torch.where(near[:, None], torch.randn(p.shape, generator=gen) * amp, p)
    assert float(margin(p).min()) >= 2.0 ** -10
    return p


def _polynomial_lookup_against_the_mirror(case, g, shared):
    """No fixture holds a polynomial lookup: the fused node (today's launches) against the plain-torch mirror on the same tensors in
    float64, with the mirror in fp32 -- the reference's operations at the reference's precision -- in the place of the reference's
    own error, at the project's rule max(4 * err_X, 2^-22 * max |X_fp64|)."""
    from motionpriorcmax_amd import ops, utils
    lk, _, times = lookup_of(g, _dev(), shared)
    p0 = _polynomial_params(g, times, len(lk.levels))
    cot = torch.from_numpy(g['g'])
    with ops.KernelTimer() as kt:
        p = p0.to(_dev()).requires_grad_(True)
        out = lk.lookup_curves(p, times, 'POLYNOMIAL')
        out.backward(cot.to(_dev()), inputs=[p])
    assert _launches(kt) == {'k_corr_lookup_fwd': 1, 'k_corr_lookup_bwd': 1}, _launches(kt)
    mirror = {}
    for dt in (torch.float32, torch.float64):
        lkc = utils.CorrLookup([lv.detach().cpu().to(dt) for lv in lk.levels], lk.num_levels_per_target, radius=lk.radius)
        pc = p0.to(dt).requires_grad_(True)
        oc = lkc.lookup_curves(pc, times, 'POLYNOMIAL')
        oc.backward(cot.to(dt), inputs=[pc])
        mirror[dt] = (oc.detach().numpy().astype('float64'), pc.grad.numpy().astype('float64'))
    for i, (name, got) in enumerate((('out', out), ('grad_params', p.grad))):
        r32, r64 = mirror[torch.float32][i], mirror[torch.float64][i]
        bound = max(4.0 * float(abs(r32 - r64).max()), 2.0 ** -22 * float(abs(r64).max()))
        check(f'{case} polynomial {name} against the float64 mirror', maxdiff(got, r64), bound)


def test_bezier_through_the_new_functions_is_bitwise_the_bezier_functions():
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_a')
    p, m = (torch.from_numpy(g[k]).to(_dev()).requires_grad_(True) for k in ('params', 'mask'))
    times, tile, scale = torch.from_numpy(g['times']), int(g['tile']), float(g['scale'])
    h, w = p.shape[-2:]
    cot = torch.from_numpy(g['g']).to(_dev())
    a, _ = utils.trajectories_from_curves(p, times, tile, (8 * h, 8 * w), scale=scale, up_mask=m)
    b, _ = utils.trajectories_from_bezier(p, times, tile, (8 * h, 8 * w), scale=scale, up_mask=m)
    assert torch.equal(a, b) and _grads_equal(torch.autograd.grad(a, [p, m], cot), torch.autograd.grad(b, [p, m], cot))
    a, _ = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), 'BEZIER', None, scale)
    b, _ = utils.trajectories_from_bezier(p, times, tile, (h * tile, w * tile), scale)
    cot = torch.randn(a.shape, generator=torch.Generator().manual_seed(5)).to(_dev())
    assert torch.equal(a, b) and _grads_equal(torch.autograd.grad(a, [p], cot), torch.autograd.grad(b, [p], cot))
    with torch.no_grad():
        assert torch.equal(utils.flows_from_curves(p, times, up_mask=m, scale=scale), utils.flows_from_bezier(p, times, up_mask=m, scale=scale))
    gc = load_golden('g21_curves_corr_a')
    lk, pc, tl = lookup_of(gc, _dev())
    pc.requires_grad_(True)
    a, b = lk.lookup_curves(pc, tl), lk.lookup_bezier(pc, tl)
    cot = torch.from_numpy(gc['g']).to(_dev())
    assert torch.equal(a, b) and _grads_equal(torch.autograd.grad(a, [pc], cot), torch.autograd.grad(b, [pc], cot))


@pytest.mark.parametrize('case', ['poly3', 'learned3'])
def test_device_times_cause_no_host_synchronisation(case):
    """curve_basis on a DEVICE tensor of times -- the polynomial matrix cached per tensor, the learned one evaluated by the (frozen)
    network -- and the fused nodes forward and backward, under set_sync_debug_mode('error'); the same bits as with a list."""
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_' + case)
    dev, ct = _dev(), curve_type_of(g)
    p, m, tl, tile, shape, scale = head_inputs(g, dev)
    net = network_of(g, dev)
    if net is not None:
        net.requires_grad_(False)
    times = torch.tensor(tl, device=dev)
    cot = torch.from_numpy(g['g']).to(dev)

    def step(t):
        traj, _ = utils.trajectories_from_curves(p, t, tile, shape, ct, net, scale=scale, up_mask=m)
        return (traj.detach(),) + torch.autograd.grad(traj, [p, m], cot)

    want = step(tl)
    step(times)                                  # warm-up: the polynomial matrices of this tensor are read back once, then cached
    utils.curve_basis(ct, times, p.shape[1] // 2, net, scalar_time_shortcuts=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = step(times)
        bm = utils.curve_basis(ct, times, p.shape[1] // 2, net, scalar_time_shortcuts=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert _grads_equal(got, want)
    assert float(bm[6].abs().max()) == 0.0 and float(bm[7, -1]) == 1.0


def test_validation_metrics_of_a_learned_curve_against_the_per_scalar_fixture():
    """trajectory_val_metrics(curve_type='LEARNED') restates validation_step, which evaluates the curve once per SCALAR timestamp
    (the shortcuts of curves/base.py:98-106 at t = 0 and t = 1): against the float64 restatement of the metrics
    (tests/val_metrics_oracle.py) over the fixture's float64 per-scalar flows, at the rule of tests/test_gpu_val_metrics.py --
    |x_gpu - x_f64| <= max(4 * err_x, 2^-22 * |x_f64|), err_x the same restatement over the reference's own fp32 per-scalar flows.
    Without the shortcuts (the list behaviour) the t = 1 step differs by about the flow itself."""
    from motionpriorcmax_amd import ops, utils
    g = load_golden('g21_curves_learned3')
    dev = _dev()
    p, m, times, tile, shape, scale = head_inputs(g, dev, grad=False)
    net = network_of(g, dev)
    pred64, pred32 = torch.from_numpy(g['val_flows64']), torch.from_numpy(g['val_flows'])
    gt = O.push_off_thresholds(pred64, torch.from_numpy(g['val_gt']).clone())
    valid, E = torch.from_numpy(g['val_valid']), torch.from_numpy(g['val_event_mask'])
    want, want_up = O.metrics(pred64, gt.double(), g['times'], valid, E)
    v32, _ = O.metrics(pred32, gt, g['times'], valid, E)
    kw = dict(params=p, up_mask=m, scale=scale, flow_valid=valid.to(dev), event_mask=E.to(dev), curve_type='LEARNED', basis_network=net)
    with ops.KernelTimer() as kt:
        values, updated = utils.trajectory_val_metrics(gt.to(dev), g['times'], **kw)
    assert _launches(kt) == {'k_val_partial': 1, 'k_val_image': 1, 'k_val_final': 1}, _launches(kt)
    values, updated = {k: v.item() for k, v in values.items()}, {k: v.item() for k, v in updated.items()}
    assert updated == want_up
    for k, x in want.items():
        bound = O.bound(x, abs(v32[k] - x))
        print(f'{k}: {values[k]!r} vs {x!r}  |diff| {abs(values[k] - x):.3g} (bound {bound:.3g})')
        assert abs(values[k] - x) <= bound, (k, values[k], x, bound)
    acc = utils.TrajectoryValMetrics()
    acc.update(gt.to(dev), g['times'], **kw)
    assert {k: v.item() for k, v in acc.compute().items()}.keys() == values.keys()
    lst, _ = utils.trajectory_val_metrics(gt.to(dev), g['times'], **kw, scalar_time_shortcuts=False)
    assert abs(lst['val/epe'].item() - want['val/epe']) > 0.05 * abs(want['val/epe'])
