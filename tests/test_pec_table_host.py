"""A tabulated curve basis that trains through FocusLoss.calc_per_event_curves, host side: the definition's table gradient
(tests/pec_table_cases.py) against central finite differences, the plain-torch route of the interface against the definition on
CPU tensors, the routing rules and the argument checks of curve_type='LEARNED'.  (GPU side: tests/test_gpu_pec_table.py.)"""
import pytest
import torch
from torch import nn

import pe_curves_cases as PC
import pec_table_cases as TC
from oracle import focus_oracle as O


def _tiny(seed=0, M=300):
    """16 x 24, events 0.25 px away from pixel boundaries and well inside the image (the vote's floor and the border mask are not
    differentiable there), l2 objective."""
    shape, Bn, nb = (16, 24), 2, 3
    ev, num_pos = O.synth_events(Bn, M, shape, nb, seed=seed)
    ev[..., :2] = ev[..., :2].floor().clamp(min=2) + 0.25 + 0.5 * torch.rand(Bn, M, 2, generator=torch.Generator().manual_seed(seed + 1))
    ev[..., 0].clamp_(max=shape[0] - 3.5)
    ev[..., 1].clamp_(max=shape[1] - 3.5)
    cfg = PC.loss_cfg('l2', 'on_flow_to_tref', image_shape=shape, num_bins=nb)
    return cfg, ev, num_pos


def _mlp(d, seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, d))


def test_table_gradient_of_the_definition_against_central_differences():
    """float64, every entry of a [6, 2] table: the control points are small (0.05 px), so no event crosses a pixel boundary or a
    LUT cell within the step, and the loss is smooth in the table."""
    cfg, ev, num_pos = _tiny()
    d, S, eps = 2, 5, 1e-6
    g = torch.Generator().manual_seed(4)
    params = (torch.randn(2, 2 * d, 4, 6, generator=g) * 0.05).double()
    table = (torch.randn(S + 1, d, generator=g) * 0.5).double()
    r = TC.definition(cfg, ev, num_pos, params, None, table, 0.41, dtype=torch.float64)
    got = r['g_table']
    assert float(got.abs().max()) > 0
    fd = torch.zeros_like(table)
    for i in range(S + 1):
        for j in range(d):
            lo, hi = table.clone(), table.clone()
            lo[i, j] -= eps
            hi[i, j] += eps
            fd[i, j] = (TC.definition(cfg, ev, num_pos, params, None, hi, 0.41, dtype=torch.float64)['loss']
                        - TC.definition(cfg, ev, num_pos, params, None, lo, 0.41, dtype=torch.float64)['loss']) / (2 * eps)
    err = (got - fd).abs().max() / fd.abs().max()
    print(f'table gradient against central differences: {float(err):.3e} of the largest entry')
    assert err < 1e-6
    # both parts are there: without the smoothness term the gradient is another one
    r0 = TC.definition(dict(cfg, smooth_weight=0.0), ev, num_pos, params, None, table, 0.41, dtype=torch.float64)
    assert float((r0['g_table'] - got).abs().max()) > 0 and float(r0['g_table'].abs().max()) > 0


class _Prewarped:
    """ops.PrewarpedFocusFn on CPU tensors, from the oracle's blocks (differentiable)."""
    cfg = None

    @classmethod
    def apply(cls, warped, events, t_ref, pcfg, num_pos):
        c = cls.cfg
        iwes, _ = O.make_iwes(events, warped[:, None], t_ref, tuple(c['image_shape']), c['scale_iwe_by_dt'], c['mask_image_border'],
                              c['polarity_aware_batching'], num_pos)
        return 1 / O.contrast_value(iwes, c.get('loss_type', 'gradient_magnitude'), c['focus_loss_norm']), iwes.detach()


class _LutSmooth:
    @staticmethod
    def apply(field, pcfg, weight):
        return weight * O.smoothness(field.permute(0, 3, 1, 2))


@pytest.mark.parametrize('smooth_type', ['on_flow_to_tref', 'on_flow_to_next'])
def test_the_interface_on_cpu_tensors_returns_the_table_gradient_of_the_definition(monkeypatch, smooth_type):
    """CPU tensors take the plain-torch route with phi and phim in the graph; the two GPU nodes around it (vote + objective,
    Charbonnier term) are stood in for by the oracle's blocks.  All three gradients match the definition."""
    from motionpriorcmax_amd import LossFactory, ops
    cfg, ev, num_pos = _tiny(seed=3)
    cfg = dict(cfg, smooth_type=smooth_type)
    d, S = 3, 7
    g = torch.Generator().manual_seed(5)
    params = torch.randn(2, 2 * d, 2, 3, generator=g) * 0.1
    mask = torch.randn(2, 576, 2, 3, generator=g)
    table = torch.randn(S + 1, d, generator=g) * 0.5
    _Prewarped.cfg = cfg
    monkeypatch.setattr(ops, 'PrewarpedFocusFn', _Prewarped)
    monkeypatch.setattr(ops, 'LutSmoothFn', _LutSmooth)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    p, m, tb = params.clone().requires_grad_(True), mask.clone().requires_grad_(True), table.clone().requires_grad_(True)
    loss, _, misc = L.calc_per_event_curves(p, 0.41, {'events': ev, 'num_pos_events': num_pos}, up_mask=m, curve_type='TABLE', basis_table=tb)
    loss.backward()
    assert tb.grad is not None and torch.isfinite(tb.grad).all() and float(tb.grad.abs().max()) > 0
    r64 = TC.definition(cfg, ev, num_pos, params, mask, table, 0.41, dtype=torch.float64)
    assert abs(float(loss.detach()) - float(r64['loss'])) <= 1e-5 * abs(float(r64['loss']))
    for what, got, want in (('table', tb.grad, r64['g_table']), ('params', p.grad, r64['g_params']), ('up_mask', m.grad, r64['g_mask'])):
        r = TC.rel(got, want)
        print(f'{smooth_type}: {what} gradient, relative L2 to the float64 definition {r:.3e}')
        assert r < 1e-4, what


def test_routing_of_constant_and_trainable_tables(monkeypatch):
    """A constant table still reaches ops.PerEventCurvesFn with its twelve arguments and a detached table; a trainable one reaches
    it un-detached where pec_supported answers 1, and the in-graph plain-torch chain (GatherRowsFn, PrewarpedFocusFn) where it
    answers 0."""
    from motionpriorcmax_amd import LossFactory, ops
    L = LossFactory.get_loss_calculator('FOCUS', PC.loss_cfg(smooth_weight=0.0))
    Ls = LossFactory.get_loss_calculator('FOCUS', PC.loss_cfg())
    ev, num_pos = O.synth_events(2, 50, PC.SHAPE, PC.NB, seed=1)
    batch = {'events': ev, 'num_pos_events': num_pos}
    seen = []

    class Fused:
        @staticmethod
        def apply(params, up_mask, events, t_ref, phim, cfg, num_pos, offsets, curve_type, table, scale, tile):
            seen.append(('fused', curve_type, table.requires_grad, None if phim is None else phim.requires_grad))
            z = torch.zeros(())
            return z, z, z, torch.zeros(2, 2, *PC.SHAPE)

    class Unfused:
        @staticmethod
        def apply(c_rows, events, phi, t_ref, cfg, num_pos, offsets=None):
            seen.append(('unfused', phi.requires_grad))
            return torch.zeros(()), torch.zeros(2, 2, *PC.SHAPE)

    class Prewarped:
        @staticmethod
        def apply(warped, events, t_ref, cfg, num_pos):
            seen.append(('in-graph', warped.requires_grad, tuple(warped.shape)))
            return warped.sum() * 0, torch.zeros(2, 2, *PC.SHAPE)

    served = [3]
    monkeypatch.setattr(ops, 'PerEventCurvesFn', Fused)
    monkeypatch.setattr(ops, 'PerEventBasisFocusFn', Unfused)
    monkeypatch.setattr(ops, 'PrewarpedFocusFn', Prewarped)
    monkeypatch.setattr(ops, 'LutSmoothFn', _LutSmooth)
    monkeypatch.setattr(ops, 'pec_supported', lambda cfg, events, num_pos, d, curve_type, samples=0: served[0])
    p = torch.zeros(2, 6, PC.HQ, PC.WQ)
    const, train = torch.zeros(65, 3), torch.randn(65, 3).requires_grad_(True)
    L.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=const)
    assert seen[-1] == ('fused', 'TABLE', False, None)
    L.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=train)
    assert seen[-1] == ('fused', 'TABLE', True, None)
    Ls.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=train)
    assert seen[-1] == ('fused', 'TABLE', True, True)                     # (phim is built in the graph)
    Ls.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=const)
    assert seen[-1] == ('fused', 'TABLE', False, False)
    with torch.no_grad():                                                 # (grad mode off: a constant)
        Ls.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=train)
    assert seen[-1] == ('fused', 'TABLE', False, False)
    served[0] = 0
    L.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=const)
    assert seen[-1] == ('unfused', False)
    loss, _, _ = Ls.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=train)
    assert seen[-1] == ('in-graph', True, (2, 50, 2)) and loss.requires_grad
    served[0] = 3
    L.calc_per_event_curves(p, 0.4, batch, curve_type='TABLE', basis_table=train, fused=False)
    assert seen[-1] == ('in-graph', True, (2, 50, 2))
    # 'LEARNED' is the 'TABLE' route with the network at the knots, inside the graph
    net = _mlp(3)
    L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED', basis_network=net, table_samples=16)
    assert seen[-1] == ('fused', 'TABLE', True, None)
    for q in net.parameters():
        q.requires_grad_(False)
    L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED', basis_network=net)
    assert seen[-1] == ('fused', 'TABLE', False, None)


def test_learned_table_is_the_network_at_the_knots(monkeypatch):
    from motionpriorcmax_amd import LossFactory, ops
    from motionpriorcmax_amd.utils import curve_basis
    L = LossFactory.get_loss_calculator('FOCUS', PC.loss_cfg(smooth_weight=0.0))
    ev, num_pos = O.synth_events(2, 50, PC.SHAPE, PC.NB, seed=1)
    got = []

    class Fused:
        @staticmethod
        def apply(params, up_mask, events, t_ref, phim, cfg, num_pos, offsets, curve_type, table, scale, tile):
            got.append(table)
            z = torch.zeros(())
            return z, z, z, torch.zeros(2, 2, *PC.SHAPE)

    monkeypatch.setattr(ops, 'PerEventCurvesFn', Fused)
    monkeypatch.setattr(ops, 'pec_supported', lambda *a, **k: 3)
    net = _mlp(3)
    L.calc_per_event_curves(torch.zeros(2, 6, PC.HQ, PC.WQ), 0.4, {'events': ev, 'num_pos_events': num_pos}, curve_type='LEARNED',
                            basis_network=net, table_samples=37)
    want = curve_basis('LEARNED', torch.arange(38, dtype=torch.float32) / 37, 3, net)
    assert tuple(got[0].shape) == (38, 3) and torch.equal(got[0], want) and got[0].requires_grad


def test_learned_argument_checks():
    from motionpriorcmax_amd import LossFactory
    L = LossFactory.get_loss_calculator('FOCUS', PC.loss_cfg())
    ev, num_pos = O.synth_events(2, 50, PC.SHAPE, PC.NB, seed=1)
    batch = {'events': ev, 'num_pos_events': num_pos}
    p = torch.zeros(2, 6, PC.HQ, PC.WQ)
    with pytest.raises(ValueError, match='basis_network'):
        L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED')
    with pytest.raises(ValueError, match='degree'):
        L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED', basis_network=_mlp(4))        # wrong output width
    with pytest.raises(ValueError, match='table_samples'):
        L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED', basis_network=_mlp(3), table_samples=0)
    with pytest.raises(ValueError, match='basis_table'):
        L.calc_per_event_curves(p, 0.4, batch, curve_type='LEARNED', basis_network=_mlp(3), basis_table=torch.zeros(9, 3))
