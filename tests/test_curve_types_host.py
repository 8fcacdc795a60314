"""The reference's other two RAFT-spline curve types on the host: utils.curve_basis and the plain-torch mirrors behind
utils.trajectories_from_curves / flows_from_curves / CorrLookup.lookup_curves on CPU tensors, against the g21_curves fixtures
(tools/gen_golden_curves.py: the unmodified reference's PolynomialCurves / LearnedCurves with the basis network of
src/modules/raft_spline.py:29-34 in fp32, a float64 evaluation of the same formulas and the measured distance between the two).

Tolerance rules (shared with tests/test_gpu_curve_types.py), nothing fixed in advance:
  every tensor the Bezier nodes produce too   max |X - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|), err_X = max |X_reference_fp32 -
                                              X_fp64| from the fixture (tests/test_cvx_traj_host.py); `traj` gets half an ulp of its
                                              largest coordinate on top of the flows' tolerance for its one add
  grad_basis, per element                     max(4 * err_X, (2 + ceil(log2 N)) * 2^-24 * S): S the float64 sum of the element's absolute
                                              addends and N their count (fixture); one rounding for the product, one for the scale,
                                              and the depth of a balanced tree over the N addends
  the network's parameter gradients           the same with S_theta = sum_(t, j) |d basis[t, j] / d theta| * S[t, j] (fixture): autograd
                                              carries grad_basis into them linearly, so its error arrives weighted by |Jacobian|."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

HEAD_CASES = ['poly1', 'poly3', 'learned1', 'learned3', 'learned16', 'learned10']
LEARNED_HEAD_CASES = [c for c in HEAD_CASES if c.startswith('learned')]
CORR_CASES = ['corr_a', 'corr_b', 'corr_c']


def tol(g, name):
    return max(4.0 * float(g['err_' + name]), 2.0 ** -22 * float(np.abs(g[name + '64']).max()))


def tol_traj(g, suffix=''):
    return tol(g, 'flows') + float(np.spacing(np.float32(np.abs(g['traj' + suffix + '64']).max()))) / 2


def tol_sum(g, name, s_name, n_name):
    """Per element: max(4 * err_X, (2 + ceil(log2 N)) * 2^-24 * S)."""
    depth = math.ceil(math.log2(int(g[n_name])))
    return np.maximum(4.0 * float(g['err_' + name]), (2 + depth) * 2.0 ** -24 * g[s_name])


def maxdiff(t, ref64):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - ref64).max())


def check(label, got, bound):
    print(f'{label}: {got:.4g} (bound {bound:.4g})')
    assert got <= bound, (label, got, bound)


def check_elementwise(label, t, ref64, bound):
    """Every element within its own bound; prints the largest ratio."""
    diff = np.abs(t.detach().cpu().numpy().astype(np.float64) - ref64)
    ratio = diff / np.maximum(bound, np.finfo(np.float64).tiny)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    print(f'{label}: max |diff| {float(diff.max()) if diff.size else 0.0:.4g}, largest diff / bound {float(ratio[i]) if ratio.size else 0.0:.4g} '
          f'(bound there {float(np.broadcast_to(bound, diff.shape)[i]) if ratio.size else 0.0:.4g})')
    assert (diff <= bound).all(), (label, float(diff.max()))


def curve_type_of(g):
    return str(g['curve_type'])


def network_of(g, device='cpu'):
    """The basis network of reference src/modules/raft_spline.py:29-34 with the fixture's weights (None for a polynomial case)."""
    if 'net_0' not in g:
        return None
    d = g['net_4'].shape[0]
    net = torch.nn.Sequential(torch.nn.Linear(1, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, d))
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.from_numpy(g[f'net_{i}']))
    return net.to(device)


class BasisTap:
    """Keeps the network's latest output and has autograd retain its gradient: the basis matrix the entry points form inside."""

    def __init__(self, net):
        self.out = None
        self.handle = net.register_forward_hook(self)

    def __call__(self, module, inputs, output):
        if output.requires_grad:
            output.retain_grad()
        self.out = output


def head_inputs(g, device='cpu', grad=True):
    p = torch.from_numpy(g['params']).to(device).requires_grad_(grad)
    m = torch.from_numpy(g['mask']).to(device).requires_grad_(grad)
    h, w = p.shape[-2:]
    return p, m, [float(t) for t in g['times']], int(g['tile']), (8 * h, 8 * w), float(g['scale'])


def run_head(g, device='cpu', plain=False, params_grad=True, times=None, frozen=False):
    """trajectories_from_curves and every gradient autograd can give -> dict(traj, pos, grad_params, grad_mask, grad_basis, grad_net);
    `frozen`: the network's parameters do not require grad (the basis matrix is a constant)."""
    from motionpriorcmax_amd import utils
    p, m, tl, tile, shape, scale = head_inputs(g, device)
    if not params_grad:
        p = p.detach()
    net = network_of(g, device)
    if frozen and net is not None:
        net.requires_grad_(False)
    tap = BasisTap(net) if net is not None else None
    times = tl if times is None else times
    if plain:
        h, w = p.shape[-2:]
        traj, pos = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), curve_type_of(g), net, scale=scale)
        cot = torch.from_numpy(g['g_plain']).to(device)
        leaves = [p] if params_grad else []
    else:
        traj, pos = utils.trajectories_from_curves(p, times, tile, shape, curve_type_of(g), net, scale=scale, up_mask=m)
        cot = torch.from_numpy(g['g']).to(device)
        leaves = ([p] if params_grad else []) + [m]
    res = dict(traj=traj, pos=pos, grad_params=None, grad_mask=None, grad_basis=None, grad_net=None, net=net)
    traj.backward(cot, inputs=leaves + (list(net.parameters()) if net is not None and not frozen else []))
    if params_grad:
        res['grad_params'] = p.grad
    if not plain:
        res['grad_mask'] = m.grad
    if frozen:
        res['net'] = None
    elif net is not None:
        res['grad_basis'] = tap.out.grad
        res['grad_net'] = [q.grad for q in net.parameters()]
        tap.handle.remove()
    return res


def check_head(case, g, res, plain):
    sfx = '_plain' if plain else ''
    assert res['traj'].dtype == torch.float32 and res['traj'].shape == g['traj' + sfx + '64'].shape
    check(f'{case}{sfx} traj', maxdiff(res['traj'], g['traj' + sfx + '64']), tol_traj(g, sfx))
    check(f'{case}{sfx} grad_params', maxdiff(res['grad_params'], g['grad_params' + sfx + '64']), tol(g, 'grad_params' + sfx))
    if not plain:
        check(f'{case} grad_mask', maxdiff(res['grad_mask'], g['grad_mask64']), tol(g, 'grad_mask'))
        assert float(res['grad_mask'].detach().cpu()[torch.from_numpy(g['grad_mask64'] == 0)].abs().max()) == 0.0
    if res['net'] is not None:
        n_name = 'N_grad_basis' + sfx
        check_elementwise(f'{case}{sfx} grad_basis (N = {int(g[n_name])})', res['grad_basis'], g['grad_basis' + sfx + '64'],
                          tol_sum(g, 'grad_basis' + sfx, 'S_grad_basis' + sfx, n_name))
        for i, gn in enumerate(res['grad_net']):
            name = f'grad_net{sfx}_{i}'
            check_elementwise(f'{case} {name}', gn, g[name + '64'], tol_sum(g, name, f'S_grad_net{sfx}_{i}', n_name))


@pytest.mark.parametrize('plain', [False, True])
@pytest.mark.parametrize('case', HEAD_CASES)
def test_mirror_matches_the_fixtures(case, plain):
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_' + case)
    res = run_head(g, plain=plain)
    check_head(case, g, res, plain)
    if not plain:
        p, m, times, tile, shape, scale = head_inputs(g, grad=False)
        assert torch.equal(res['pos'], torch.nonzero(utils.get_optical_flow_tile_mask(shape, tile)))
        flows = utils.flows_from_curves(p, times, curve_type_of(g), network_of(g), up_mask=m, scale=scale)
        assert flows.shape == (len(times),) + g['flows64'].shape[1:]
        check(f'{case} flows', maxdiff(flows[g['flow_times']], g['flows64']), tol(g, 'flows'))


@pytest.mark.parametrize('case', HEAD_CASES)
def test_curve_basis_rows_are_the_reference_values(case):
    """List behaviour: the rows the reference evaluates (also at t = 0 and t = 1: a learned basis is not zero at 0).  With the
    scalar-time shortcuts: the t = 0 row all zeros, the t = 1 row one-hot on the last column, every other row unchanged."""
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_' + case)
    ct, net, times = curve_type_of(g), network_of(g), [float(t) for t in g['times']]
    d = g['basis'].shape[1]
    assert times[6] == 0.0 and times[7] == 1.0
    bm = utils.curve_basis(ct, times, d, net)
    assert bm.dtype == torch.float32 and tuple(bm.shape) == (8, d)
    if ct == 'POLYNOMIAL':
        assert torch.equal(bm, torch.from_numpy(g['basis'])) and not bm.requires_grad
    else:
        assert bm.requires_grad
        assert float(bm[6].detach().abs().max()) > 0.0
    check(f'{case} basis', maxdiff(bm, g['basis64']), tol(g, 'basis'))
    sc = utils.curve_basis(ct, times, d, net, scalar_time_shortcuts=True)
    assert torch.equal(sc[:6], bm[:6].detach() if ct == 'POLYNOMIAL' else bm[:6])
    assert torch.equal(sc[6].detach(), torch.zeros(d))
    assert torch.equal(sc[7].detach(), torch.nn.functional.one_hot(torch.tensor(d - 1), d).float())
    if ct == 'LEARNED':                          # the shortcut rows are constants: no gradient reaches the network through them
        (gb,) = torch.autograd.grad(sc.sum(), net[4].bias)
        assert torch.equal(gb, torch.full((d,), 6.0))
        t = torch.tensor(times)
        assert torch.equal(utils.curve_basis(ct, t, d, net), bm)          # a tensor of times: the same rows


def test_the_shortcuts_compare_the_times_before_they_are_rounded_to_fp32():
    """The reference compares the Python float with 0 and 1 (curves/base.py:102-105) and rounds to fp32 afterwards: 1 - 1e-12 and
    1e-320 get no shortcut although the basis is then evaluated at 1.0f and 0.0f; a tensor is compared in its own dtype."""
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_learned3')
    net = network_of(g)
    times = [0.0, 1e-320, 1.0 - 1e-12, 1.0]
    assert np.float32(times[1]) == 0.0 and np.float32(times[2]) == 1.0
    for ct, nw in (('POLYNOMIAL', None), ('LEARNED', net)):
        for tt in (times, np.asarray(times), torch.tensor(times, dtype=torch.float64)):
            lst = utils.curve_basis(ct, tt, 3, nw).detach()
            sc = utils.curve_basis(ct, tt, 3, nw, scalar_time_shortcuts=True).detach()
            assert torch.equal(sc[0], torch.zeros(3)) and torch.equal(sc[3], torch.tensor([0.0, 0.0, 1.0]))
            assert torch.equal(sc[1:3], lst[1:3]) and torch.equal(lst[1], lst[0]) and torch.equal(lst[2], lst[3])
        sc = utils.curve_basis(ct, torch.tensor(times, dtype=torch.float32), 3, nw, scalar_time_shortcuts=True).detach()
        assert torch.equal(sc[:2], torch.zeros(2, 3)) and torch.equal(sc[2:], torch.tensor([[0.0, 0.0, 1.0]] * 2))


def test_the_validation_rows_are_what_the_reference_evaluates_per_scalar():
    """flows_from_curves over the shortcut matrix is the reference's per-scalar evaluation (validation_step); over the list matrix it
    is not, at t = 1, by about the size of the flow itself."""
    from motionpriorcmax_amd import utils
    from motionpriorcmax_amd.utils.basis import _cvx_upsample
    g = load_golden('g21_curves_learned3')
    p, m, times, tile, shape, scale = head_inputs(g, grad=False)
    net = network_of(g)
    with torch.no_grad():
        up = _cvx_upsample(p, m).reshape(p.shape[0], 2, 3, *shape)
        val = torch.einsum('bcdhw,td->tbchw', up, utils.curve_basis('LEARNED', times, 3, net, scalar_time_shortcuts=True)) * scale
        lst = utils.flows_from_curves(p, times, 'LEARNED', net, up_mask=m, scale=scale)
    check('val_flows (shortcut rows)', maxdiff(val, g['val_flows64']), tol(g, 'val_flows'))
    check('basis with shortcut rows', maxdiff(utils.curve_basis('LEARNED', times, 3, net, scalar_time_shortcuts=True), g['basis_val64']), tol(g, 'basis'))
    assert maxdiff(lst[7], g['val_flows64'][7]) > 0.1 * float(np.abs(g['val_flows64'][7]).max())
    assert maxdiff(lst[6], g['val_flows64'][6]) > 0.0 and float(np.abs(g['val_flows64'][6]).max()) == 0.0


def test_bezier_is_the_bernstein_matrix_and_the_bezier_functions_bitwise():
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_a')
    times = torch.from_numpy(g['times'])
    for d in (1, 3, 10, 16):
        assert torch.equal(utils.curve_basis('BEZIER', times, d), utils.bernstein_basis(times, d))
        assert torch.equal(utils.curve_basis('BEZIER', list(g['times']), d, scalar_time_shortcuts=True), utils.bernstein_basis(times, d))
    p, m = torch.from_numpy(g['params']), torch.from_numpy(g['mask'])
    h, w = p.shape[-2:]
    tile, scale = int(g['tile']), float(g['scale'])
    a, pa = utils.trajectories_from_curves(p, times, tile, (8 * h, 8 * w), scale=scale, up_mask=m)
    b, pb = utils.trajectories_from_bezier(p, times, tile, (8 * h, 8 * w), scale=scale, up_mask=m)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    a, _ = utils.trajectories_from_curves(p, times, tile, (h * tile, w * tile), 'BEZIER', None, scale)
    b, _ = utils.trajectories_from_bezier(p, times, tile, (h * tile, w * tile), scale)
    assert torch.equal(a, b)
    assert torch.equal(utils.flows_from_curves(p, times, up_mask=m, scale=scale), utils.flows_from_bezier(p, times, up_mask=m, scale=scale))
    assert torch.equal(utils.flows_from_curves(p, times), utils.flows_from_bezier(p, times))


def test_argument_errors():
    from motionpriorcmax_amd import utils
    g = load_golden('g21_curves_learned3')
    p, m, times, tile, shape, scale = head_inputs(g, grad=False)
    net = network_of(g)
    for bad in ('bezier', 'LEARNED_2D', '', None):
        with pytest.raises(ValueError):
            utils.curve_basis(bad, times, 3, net)
        with pytest.raises(ValueError):
            utils.trajectories_from_curves(p, times, tile, shape, bad, net, up_mask=m)
    with pytest.raises(ValueError):
        utils.curve_basis('LEARNED', times, 3)                             # no network
    with pytest.raises(ValueError):
        utils.curve_basis('LEARNED', times, 4, net)                        # a network of another degree
    with pytest.raises(ValueError):
        utils.curve_basis('POLYNOMIAL', times, 0)
    with pytest.raises(ValueError):
        utils.trajectories_from_curves(p, times, tile, (8, 8), 'LEARNED', net, up_mask=m)
    with pytest.raises(ValueError):
        utils.flows_from_curves(p, times, 'LEARNED', net, up_mask=m[:, :9])
    gt = torch.zeros(2, 8, 2, *shape)
    with pytest.raises(ValueError):
        utils.trajectory_val_metrics(gt, times, params=p, up_mask=m, event_mask=torch.ones(2, *shape, dtype=torch.bool), curve_type='SPLINE')
    with pytest.raises(ValueError):
        utils.trajectory_val_metrics(gt, times, params=p, up_mask=m, event_mask=torch.ones(2, *shape, dtype=torch.bool), curve_type='LEARNED')


# ---------------------------------------------------------------- the correlation lookup

def lookup_of(g, device='cpu', shared_grad=False):
    """(CorrLookup over the pyramid rebuilt from the fixture's feature maps -- exact in fp32 --, params, times as a list)."""
    from motionpriorcmax_amd import utils
    nl = [int(v) for v in g['num_levels']]
    levels, _ = utils.corr_pyramid(torch.from_numpy(g['fmap1']).to(device), torch.from_numpy(g['fmap2']).to(device), nl)
    levels = [lv.detach().requires_grad_(shared_grad) for lv in levels]
    return utils.CorrLookup(levels, nl, radius=int(g['radius']), shared_grad=shared_grad), torch.from_numpy(g['params']).to(device), [float(t) for t in g['times']]


def run_lookup(g, device='cpu', params_grad=True, shared_grad=False, times=None, frozen=False):
    lk, p, tl = lookup_of(g, device, shared_grad)
    p.requires_grad_(params_grad)
    net = network_of(g, device).requires_grad_(not frozen)
    tap = BasisTap(net)
    out = lk.lookup_curves(p, tl if times is None else times, 'LEARNED', net)
    out.backward(torch.from_numpy(g['g']).to(device), inputs=([p] if params_grad else []) + ([] if frozen else list(net.parameters())))
    tap.handle.remove()
    return dict(out=out, grad_params=p.grad, grad_basis=tap.out.grad, grad_net=[q.grad for q in net.parameters()], net=None if frozen else net, lookup=lk)


def check_lookup(case, g, res):
    check(f'{case} out', maxdiff(res['out'], g['out64']), tol(g, 'out'))
    check(f'{case} grad_params', maxdiff(res['grad_params'], g['grad_params64']), tol(g, 'grad_params'))
    z = torch.from_numpy(g['grad_params64'] == 0)
    if bool(z.any()):
        assert float(res['grad_params'].detach().cpu()[z].abs().max()) == 0.0
    if res['net'] is None:
        return
    check_elementwise(f"{case} grad_basis (N = {int(g['N_grad_basis'])})", res['grad_basis'], g['grad_basis64'],
                      tol_sum(g, 'grad_basis', 'S_grad_basis', 'N_grad_basis'))
    for i, gn in enumerate(res['grad_net']):
        check_elementwise(f'{case} grad_net_{i}', gn, g[f'grad_net_{i}64'], tol_sum(g, f'grad_net_{i}', f'S_grad_net_{i}', 'N_grad_basis'))


@pytest.mark.parametrize('case', CORR_CASES)
def test_lookup_mirror_matches_the_fixtures(case):
    g = load_golden('g21_curves_' + case)
    check_lookup(case, g, run_lookup(g))


def test_lookup_curves_with_bezier_is_lookup_bezier():
    g = load_golden('g21_curves_corr_a')
    lk, p, times = lookup_of(g)
    assert torch.equal(lk.lookup_curves(p, times), lk.lookup_bezier(p, times))
    with pytest.raises(ValueError):
        lk.lookup_curves(p, times, 'CUBIC')
    with pytest.raises(ValueError):
        lk.lookup_curves(p, times[:1], 'POLYNOMIAL')
