"""A tabulated curve basis that TRAINS through FocusLoss.calc_per_event_curves on the GPU (csrc/pe_curves.hip: k_pec_table_grad,
mpc_pec_field_basis_grad; the shared body in csrc/pe_device.h) against the DEFINITION in tests/pec_table_cases.py, fp32 and
float64, bit for bit across runs, layouts and against the sibling family's kernel, and at its edges.  (Host side:
tests/test_pec_table_host.py.)"""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import pe_curves_cases as PC
import pec_table_cases as TC
from oracle import focus_oracle as O

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def _loss(cfg):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _step(L, params, mask, table, t_ref, batch, scale=1.0, fused=True, tap=False, trains=True, learned=None):
    """One forward + backward on the device -> dict(loss, iwes, g_params, g_mask, g_table, g_rows).  `learned` = (network on the
    device, samples): curve_type='LEARNED', and g_table is the flattened gradient of the network's parameters."""
    from motionpriorcmax_amd import ops
    dev = batch['events'].device
    pg = params.to(dev).requires_grad_(True)
    mg = mask.to(dev).requires_grad_(True) if mask is not None else None
    ops.PEC_ROWS_GRAD_TAP = [] if tap else None
    try:
        if learned is not None:
            net, S = learned
            loss, _, misc = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type='LEARNED', basis_network=net, table_samples=S,
                                                    scale=scale, fused=fused)
            wrt = [pg] + ([mg] if mg is not None else []) + list(net.parameters())
            gs = torch.autograd.grad(loss, wrt)
            gp, gm = gs[0], (gs[1] if mg is not None else None)
            gt = torch.cat([g.reshape(-1) for g in gs[(2 if mg is not None else 1):]])
        else:
            tb = table.to(dev).requires_grad_(bool(trains))
            loss, _, misc = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type='TABLE', basis_table=tb, scale=scale, fused=fused)
            loss.backward()
            gp, gm, gt = pg.grad, (mg.grad if mg is not None else None), tb.grad
        g_rows = ops.PEC_ROWS_GRAD_TAP[0] if (tap and ops.PEC_ROWS_GRAD_TAP) else None
    finally:
        ops.PEC_ROWS_GRAD_TAP = None
    return dict(loss=loss.detach(), iwes=misc['iwes'], g_params=gp, g_mask=gm, g_table=gt, g_rows=g_rows)


def _against(label, cfg, ev, num_pos, out, r32, r64, loss_finite=True):
    """The rules of the feature's issue: loss 1e-5, IWEs 1e-5 * max, params and up_mask as the curve tests hold them, the table by
    pec_table_cases.table_rule."""
    bound = TC.bound_of(cfg)
    if loss_finite:
        # (loss and IWEs against the fp32 definition, as tests/test_gpu_pe_table.py holds them: the basis is DEFINED by five fp32
        # operations, which the kernels repeat bit for bit.  Only test_limits needs it: at S = 16383 the rounding of t * S alone
        # moves an fp32 IWE by 1.5e-5 of its maximum from the float64 one.  The gradients below are held to float64.)
        l32, l64 = float(r32['loss']), float(r64['loss'])
        iw = r32['iwes'].reshape(out['iwes'].shape)
        d_iw = float((out['iwes'].cpu() - iw).abs().max() / iw.abs().max())
        print(f'PEC_TABLE | {label} | loss {out["loss"].item():.9g} against {l32:.9g} (float64 {l64:.9g}) | IWEs {d_iw:.3e} of the maximum')
        assert abs(out['loss'].item() - l32) <= 1e-5 * abs(l32), label
        assert d_iw <= 1e-5, label
    gp = out['g_params'].cpu()
    assert torch.isfinite(gp).all(), label
    grads = [('params', gp, r32['g_params'], r64['g_params'])]
    if out['g_mask'] is not None:
        assert torch.isfinite(out['g_mask']).all(), label
        grads.append(('up_mask', out['g_mask'].cpu(), r32['g_mask'], r64['g_mask']))
    if TC.sign_free(cfg):
        for what, got, _, g64 in grads:
            r = TC.rel(got, g64)
            print(f'PEC_TABLE | {label} | {what} | to float64 {r:.3e}')
            assert r < 1e-4, (label, what, r)
    elif out['g_rows'] is not None:
        TC.rows_accounting(cfg, ev, num_pos, r64, out['g_rows'].cpu(), label)
    else:
        # (the 'l1' objective on the plain-torch route: no node hands out a rows gradient to account for, so params and up_mask are
        # held as tests/test_gpu_pe_table.py holds the coefficient gradient under l1 -- relative L2 to the fp32 definition below the
        # project's 2e-3, or within 4 times the fp32 definition's own distance from float64)
        for what, got, g32, g64 in grads:
            TC.grad_rule(label, what, got, g32, g64, bound)
    TC.table_rule(label, out['g_table'], r32['g_table'], r64['g_table'], bound)


def _both(cfg, ev, num_pos, params, mask, table, t_ref, scale=1.0, table_fn=None):
    return (TC.definition(cfg, ev, num_pos, params, mask, table, t_ref, scale, torch.float32, table_fn),
            TC.definition(cfg, ev, num_pos, params, mask, table, t_ref, scale, torch.float64, table_fn))


RUNS = [(n, True, None) for n in TC.CASES] + [('tab10', False, None), ('tab10_evimo', False, None), ('tab10', True, False)]


@pytest.mark.parametrize('name,fused,ordered', RUNS, ids=[f'{n}-{"fused" if f else "unfused"}{"" if o is None else "-as-loaded"}' for n, f, o in RUNS])
def test_against_the_definition(name, fused, ordered):
    """Every case on the fused node; tab10 and tab10_evimo also on the plain-torch route; tab10 also as loaded (the atomic rows
    gradient), so that both layouts meet d = 10."""
    dev = _dev()
    c = TC.CASES[name]
    cfg, ev, num_pos, params, mask, table, scale = TC.case_inputs(name)
    L = _loss(cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if c['ordered'] if ordered is None else ordered:
        batch = L.order_events(batch)
        assert 'event_offsets' in batch
    out = _step(L, params, mask, table, c['t_ref'], batch, scale, fused, tap=bool(fused))
    _against(f'{name} fused={fused} ordered={"event_offsets" in batch}', cfg, ev, num_pos, out, TC.reference(name, torch.float32),
             TC.reference(name, torch.float64))


def _time_sorted(ev, num_pos):
    """The same rows with each polarity block of each sample sorted by time, the padding rows left at the block's end."""
    out = ev.clone()
    for b in range(ev.shape[0]):
        for lo, hi in ((0, num_pos), (num_pos, ev.shape[1])):
            blk = ev[b, lo:hi]
            key = blk[:, 2].double() + 2.0 * (blk[:, 5] == 0).double()
            out[b, lo:hi] = blk[torch.argsort(key, stable=True)]
    return out


def test_table_gradient_is_bitwise_reproducible_and_a_frozen_table_runs_what_it_ran():
    dev = _dev()
    name = 'tab10_atomic'
    c = TC.CASES[name]
    cfg, ev, num_pos, params, mask, table, scale = TC.case_inputs(name)
    L = _loss(cfg)
    loaded = {'events': ev.to(dev), 'num_pos_events': num_pos}
    a, b = (_step(L, params, mask, table, c['t_ref'], loaded) for _ in range(2))
    assert torch.equal(a['g_table'], b['g_table']) and float(a['g_table'].abs().max()) > 0
    # the same events time-sorted and bucket-ordered: the same per-event products, summed in integers
    evs = _time_sorted(ev, num_pos)
    assert not torch.equal(evs, ev) and torch.equal(evs[..., 2].sort(dim=1)[0], ev[..., 2].sort(dim=1)[0])
    s = _step(L, params, mask, table, c['t_ref'], {'events': evs.to(dev), 'num_pos_events': num_pos})
    ob = L.order_events(loaded)
    o1, o2 = (_step(L, params, mask, table, c['t_ref'], ob) for _ in range(2))
    assert torch.equal(o1['g_table'], o2['g_table'])
    assert torch.equal(a['g_table'], s['g_table']) and torch.equal(a['g_table'], o1['g_table'])
    # a table that does not require grad: loss, IWEs, params and mask gradients of the trainable call, bit for bit -- and none for it
    for batch, tr in ((ob, o1), (loaded, a)):
        fz = _step(L, params, mask, table, c['t_ref'], batch, trains=False)
        assert fz['g_table'] is None
        assert torch.equal(fz['loss'], tr['loss']) and torch.equal(fz['iwes'], tr['iwes'])
        if 'event_offsets' in batch:                 # (as loaded the rows gradient adds with float atomics: not reproducible)
            assert torch.equal(fz['g_params'], tr['g_params']) and torch.equal(fz['g_mask'], tr['g_mask'])


def test_frozen_table_makes_the_launches_it_made():
    """The kernels of a step with a constant table: none of the new ones; with a trainable table the same plus the three."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    name = 'tab10'
    c = TC.CASES[name]
    cfg, ev, num_pos, params, mask, table, scale = TC.case_inputs(name)
    L = _loss(cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    with ops.KernelTimer() as k0:
        _step(L, params, mask, table, c['t_ref'], ob, trains=False)
    with ops.KernelTimer() as k1:
        _step(L, params, mask, table, c['t_ref'], ob)
    n0 = {k: v['launches'] for k, v in k0.summary().items()}
    n1 = {k: v['launches'] for k, v in k1.summary().items()}
    new = {'k_pec_table_grad': 1, 'k_pec_table_finish': 1, 'k_field_basis_grad_part': 1, 'k_field_basis_grad_sum': 1}
    assert not set(new) & set(n0), n0
    extra = {k: n1[k] - n0.get(k, 0) for k in n1 if n1[k] != n0.get(k, 0)}
    print(f'launches beside the frozen step: {extra}')
    new['k_zero_words'] = 1                      # (the zero fill of the 64-bit accumulators)
    assert extra == new and set(n0) <= set(n1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_agrees_with_the_sibling_kernel_bit_for_bit():
    """d = 3, S = 37, no mask: mpc_pec_table_basis_grad and mpc_pe_table_basis_grad through the C entry points on the same warped
    records, position gradients and rows -- both sum the same products in integers."""
    from motionpriorcmax_amd import _lib as C, ops
    dev = _dev()
    shape, sp, Bn, M, k, S = (16, 24), 4, 2, 4000, 3, 37
    L = _loss(PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=sp))
    ev, num_pos = O.synth_events(Bn, M, shape, PC.NB, seed=13, pad_frac=0.1)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    evd, offs = ob['events'], ob['event_offsets']
    sh = ops._pec_shape(L._cfg, evd, num_pos)
    n = sh.B * sh.hq * sh.wq
    g = torch.Generator().manual_seed(100 * k + S)
    rows = (torch.randn(n, 2 * k, generator=g) * 3).to(dev)
    table = torch.randn(S + 1, k, generator=g).to(dev)
    tr = torch.full((1,), 0.41, dtype=torch.float32, device=dev)
    out = torch.empty_like(evd)
    ops._call('mpc_pec_warp', dev, ctypes.byref(sh), _p(evd), _p(rows), ops.PEC_BASIS['TABLE'], k, _p(table), S, _p(tr), _p(out))
    gimg = torch.randn(Bn * 2, *shape, generator=g).to(dev)
    scal = torch.ones(C.SCAL_COUNT, dtype=torch.float32, device=dev)
    scal[C.SCAL_GCOEF] = 0.37
    go = torch.full((1,), 1.7, dtype=torch.float32, device=dev)
    g_t = torch.empty(1, n, 2 * k, device=dev)
    gpos = torch.empty(Bn, M, 2, device=dev)
    ops._call('mpc_pe_table_grad_ordered', dev, ctypes.byref(sh), _p(out), _p(offs), _p(table), S, k, _p(tr), _p(gimg), _p(scal), _p(go), _p(g_t), 1,
              _p(gpos))
    assert int((gpos != 0).any(-1).sum()) > M // 2
    got = []
    for name in ('mpc_pec_table_basis_grad', 'mpc_pe_table_basis_grad'):
        acc = torch.empty((S + 2) * k, dtype=torch.int64, device=dev)
        gt = torch.full((S + 1, k), float('nan'), device=dev)
        first = (k, S) if name == 'mpc_pec_table_basis_grad' else (S, k)
        ops._call(name, dev, ctypes.byref(sh), _p(out), _p(gpos), _p(rows), *first, _p(tr), _p(scal), _p(go), _p(acc), _p(gt))
        got.append(gt)
    print(f'table gradients differ in {int((got[0] != got[1]).sum())} of {got[0].numel()} elements')
    assert torch.isfinite(got[0]).all() and float(got[0].abs().max()) > 0
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize('S', [1, 16])
@pytest.mark.parametrize('ordered', [False, True])
def test_edges_of_the_interpolation(S, ordered):
    """The event blocks of test_gpu_pe_table.py::test_edges_of_the_interpolation -- t exactly 0, exactly 1, on knots, one ulp below
    knots and 500 events in one interval -- at d = 10; t_ref at 0, at 1, on a knot and at 0.5 / S."""
    dev = _dev()
    shape, Bn, Mn, nb, d = PC.SHAPE, 2, 12000, 5, 10
    cfg = PC.loss_cfg('l2')
    ev, num_pos = O.synth_events(Bn, Mn, shape, nb, seed=14, pad_frac=0.1)
    knots = torch.arange(S + 1, dtype=torch.float32) / S
    below = torch.from_numpy(np.nextafter(knots[1:].numpy(), np.float32(0)))
    for blk0 in (0, num_pos):                                   # in both polarity blocks
        ev[:, blk0:blk0 + 300, 2] = 0.0
        ev[:, blk0 + 300:blk0 + 600, 2] = 1.0
        ev[:, blk0 + 600:blk0 + 1100, 2] = knots[torch.arange(500) % (S + 1)]
        ev[:, blk0 + 1100:blk0 + 1600, 2] = below[torch.arange(500) % S]
        ev[:, blk0 + 1600:blk0 + 2100, 2] = (0.3 + 0.4 * torch.rand(500, generator=torch.Generator().manual_seed(1))) / S   # one interval
    ev[..., 4] = torch.clamp(torch.floor(ev[..., 2] * nb), 0, nb - 1)
    g = torch.Generator().manual_seed(7)
    params = torch.randn(Bn, 2 * d, PC.HQ, PC.WQ, generator=g) * 1.25          # (ten orders of a 0.5 table: a few pixels)
    table = torch.randn(S + 1, d, generator=g) * 0.5
    L = _loss(cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if ordered:
        bg = L.order_events(bg)
    for t_ref in (0.0, 1.0, float(knots[min(1, S)]), 0.5 / S):
        out = _step(L, params, None, table, t_ref, bg)
        r32, r64 = _both(cfg, ev, num_pos, params, None, table, t_ref)
        _against(f'edges S={S} ordered={ordered} t_ref={t_ref}', cfg, ev, num_pos, out, r32, r64)


@pytest.mark.parametrize('ordered', [False, True])
def test_rows_without_weight_contribute_exactly_nothing(ordered):
    """Rows with valid == 0 and rows that the border mask zeroes: their times change between two runs, the table gradient does not
    change in any bit."""
    dev = _dev()
    shape, Bn, Mn, nb, d, S = PC.SHAPE, 2, 12000, 5, 10, 37
    cfg = PC.loss_cfg('l2')
    ev, num_pos = O.synth_events(Bn, Mn, shape, nb, seed=15, pad_frac=0.1)
    dead = (ev[..., 5] == 0)
    assert int(dead.sum()) > 0
    far = torch.zeros(Bn, Mn, dtype=torch.bool)
    far[:, 100:400] = True
    far[:, num_pos + 100:num_pos + 400] = True
    ev[..., 0][far] = -300.0                    # far outside the image for any warp of these control points: masked by the border
    g = torch.Generator().manual_seed(8)
    params = torch.randn(Bn, 2 * d, PC.HQ, PC.WQ, generator=g) * 1.25
    table = torch.randn(S + 1, d, generator=g) * 0.5
    L = _loss(cfg)
    grads = []
    for flip in (False, True):
        e = ev.clone()
        if flip:
            e[..., 2][dead | far] = 1.0 - e[..., 2][dead | far]
        bg = {'events': e.to(dev), 'num_pos_events': num_pos}
        if ordered:
            # (the layout is that of the unflipped batch for both runs: the time bins of the rows, column 4, are left alone)
            bg = L.order_events(bg)
        grads.append(_step(L, params, None, table, 0.41, bg)['g_table'])
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_second_trip_and_ragged_tail():
    """k_pec_table_grad runs at most 256 workgroups of 1024 rows: B * M = 262 202 rows is more than 262 144 and no multiple of 1024,
    so the first workgroups make a second trip and the last one is ragged."""
    dev = _dev()
    shape, Bn, Mn, nb, d, S = (16, 24), 2, 131101, 3, 2, 9
    assert Bn * Mn > 256 * 1024 and (Bn * Mn) % 1024 != 0
    cfg = PC.loss_cfg('l2', image_shape=shape, num_bins=nb)
    ev, num_pos = O.synth_events(Bn, Mn, shape, nb, seed=17, time_sorted=True)
    g = torch.Generator().manual_seed(10)
    params = torch.randn(Bn, 2 * d, 4, 6, generator=g)
    table = torch.randn(S + 1, d, generator=g) * 0.5
    out = _step(_loss(cfg), params, None, table, 0.41, {'events': ev.to(dev), 'num_pos_events': num_pos})
    r32, r64 = _both(cfg, ev, num_pos, params, None, table, 0.41)
    _against('second trip, tiny image', cfg, ev, num_pos, out, r32, r64)


def test_no_events_the_table_gradient_is_the_smoothness_terms():
    dev = _dev()
    shape, Bn, nb, d, S = (16, 24), 2, 3, 10, 37
    cfg = PC.loss_cfg('l2', image_shape=shape, num_bins=nb)
    ev = torch.zeros(Bn, 0, 6)
    g = torch.Generator().manual_seed(11)
    params = torch.randn(Bn, 2 * d, 4, 6, generator=g) * 4.0
    table = torch.randn(S + 1, d, generator=g) * 0.5
    out = _step(_loss(cfg), params, None, table, 0.41, {'events': ev.to(dev), 'num_pos_events': 0})
    r32, r64 = _both(cfg, ev, 0, params, None, table, 0.41)
    # (an empty image has no contrast: the loss is not finite in either implementation, the gradients are the smoothness term's)
    _against('M = 0', cfg, ev, 0, out, r32, r64, loss_finite=False)


@pytest.mark.parametrize('which', ['limit', 'past', 'd17'])
def test_limits(which):
    """(S + 1) * d exactly at mpc_pe_table_limit(): the new kernel; one past it, and d = 17: the plain-torch route.  All three match
    the definition."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    shape, Bn, Mn, nb = (16, 24), 2, 300, 3
    lim = int(C.lib().mpc_pe_table_limit())
    d, S = {'limit': (1, lim - 1), 'past': (1, lim), 'd17': (17, 37)}[which]
    cfg = PC.loss_cfg('l2', image_shape=shape, num_bins=nb)
    ev, num_pos = O.synth_events(Bn, Mn, shape, nb, seed=18)
    g = torch.Generator().manual_seed(12)
    params = torch.randn(Bn, 2 * d, 4, 6, generator=g) * (2.0 if d == 1 else 0.5)
    table = torch.cumsum(torch.randn(S + 1, d, generator=g) * 0.02, 0) if d == 1 else torch.randn(S + 1, d, generator=g) * 0.5
    L = _loss(cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    served = which == 'limit'
    assert bool(ops.pec_supported(L._cfg, bg['events'], num_pos, d, 'TABLE', S) & 1) == served
    with ops.KernelTimer() as kt:
        out = _step(L, params, None, table, 0.41, bg)
    names = set(kt.summary())
    assert ('k_pec_table_grad' in names) == served and ('k_pec_warp' in names) == served, names
    r32, r64 = _both(cfg, ev, num_pos, params, None, table, 0.41)
    _against(f'limits: {which}', cfg, ev, num_pos, out, r32, r64)


def _mlp(d, seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, d))


def test_learned_curves_train_end_to_end():
    """The reference's basis network (1 -> 64 -> 64 -> 64 -> d, LeakyReLU), d = 10, at 257 knots through curve_type='LEARNED': every
    parameter gets a finite non-zero gradient, and the flattened parameter gradient matches the definition run through the same
    network on the CPU."""
    dev = _dev()
    d, S = 10, 256
    cfg = PC.loss_cfg('l2')
    ev, num_pos = O.synth_events(PC.B, PC.M, PC.SHAPE, PC.NB, seed=13, pad_frac=0.1)
    g = torch.Generator().manual_seed(6)
    params = torch.randn(PC.B, 2 * d, 12, 16, generator=g) * 0.5
    mask = torch.randn(PC.B, 576, 12, 16, generator=g)
    net = _mlp(d)
    L = _loss(cfg)
    bg = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    nd = _mlp(d).to(dev)
    nd.load_state_dict(net.state_dict())

    def on_host(dtype):
        n = _mlp(d).to(dtype)
        n.load_state_dict(net.state_dict())
        knots = torch.arange(S + 1, dtype=torch.float32).to(dtype) / S
        return n(knots[:, None]), list(n.parameters())
    out = _step(L, params, mask, None, 0.41, bg, learned=(nd, S))
    sizes = [p.numel() for p in net.parameters()]
    for gpart in torch.split(out['g_table'].cpu(), sizes):
        assert torch.isfinite(gpart).all() and float(gpart.abs().max()) > 0
    r32, r64 = _both(cfg, ev, num_pos, params, mask, None, 0.41, table_fn=on_host)
    # (the flattened parameter gradient has no knot rows: the whole, by the rule of the table gradient)
    out['g_table'] = out['g_table'].cpu()
    TC.grad_rule('learned curves, S=256', 'network parameters', out['g_table'], r32['g_table'], r64['g_table'], TC.bound_of(cfg))
    l32 = float(r32['loss'])
    assert abs(out['loss'].item() - l32) <= 1e-5 * abs(l32)
    assert TC.rel(out['g_params'], r64['g_params']) < 1e-4 and TC.rel(out['g_mask'], r64['g_mask']) < 1e-4


def test_a_learned_network_on_the_cpu_still_reaches_the_fused_node():
    """curve_type='LEARNED' moves its table to the events' device inside the graph: the new kernel runs, the CPU parameters get
    their gradient."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    d, S, shape, nb = 3, 16, (16, 24), 3
    cfg = PC.loss_cfg('l2', image_shape=shape, num_bins=nb)
    ev, num_pos = O.synth_events(2, 300, shape, nb, seed=19)
    net = _mlp(d)
    pg = torch.randn(2, 2 * d, 4, 6, generator=torch.Generator().manual_seed(3)).to(dev).requires_grad_(True)
    with ops.KernelTimer() as kt:
        loss, _, _ = _loss(cfg).calc_per_event_curves(pg, 0.41, {'events': ev.to(dev), 'num_pos_events': num_pos}, curve_type='LEARNED',
                                                       basis_network=net, table_samples=S)
        loss.backward()
    assert 'k_pec_table_grad' in kt.summary(), set(kt.summary())
    for q in net.parameters():
        assert q.grad is not None and q.grad.device.type == 'cpu' and torch.isfinite(q.grad).all() and float(q.grad.abs().max()) > 0


def test_trainable_table_step_does_not_synchronise_with_the_host():
    dev = _dev()
    name = 'tab10'
    c = TC.CASES[name]
    cfg, ev, num_pos, params, mask, table, scale = TC.case_inputs(name)
    L = _loss(cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    pg, mg, tb = params.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
    t_ref = torch.full((1,), c['t_ref'], device=dev)

    def step():
        loss, _, _ = L.calc_per_event_curves(pg, t_ref, ob, up_mask=mg, curve_type='TABLE', basis_table=tb)
        loss.backward()
    step()                                       # warm-up: the one-time set-up of the kernels, the cached bin mid-times
    torch.cuda.synchronize()
    tb.grad = None
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(tb.grad).all() and float(tb.grad.abs().max()) > 0


def test_entry_points_refuse_without_a_launch():
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    lib = C.lib()
    L = _loss(PC.loss_cfg('l2', image_shape=(16, 24), num_bins=3))
    ok = ops.make_shape(L._cfg, 2, 8, 4, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
    warp = ops.make_shape(L._cfg, 2, 8, 4, 0, K=0, extra_flags=C.F_NO_BWD_RECORDS)             # without MPC_F_NO_WARP
    so, sw = ctypes.byref(ok), ctypes.byref(warp)
    # (a sentinel pattern, NaN among it: a refused call that zero-filled or wrote anything would show)
    a = (torch.arange(8192, dtype=torch.int32, device=dev) * 2654435 + 0x7FC00000).view(torch.float32)
    before = a.view(torch.int32).clone()
    assert int(torch.isnan(a).sum()) > 0
    lim = int(lib.mpc_pe_table_limit())
    P = _p(a)
    with ops.KernelTimer() as kt:
        for d, S, code in ((0, 4, C.E_SHAPE), (17, 4, C.E_UNSUPPORTED), (2, 0, C.E_SHAPE), (1, lim, C.E_UNSUPPORTED), (16, lim // 16, C.E_UNSUPPORTED)):
            assert lib.mpc_pec_table_basis_grad(so, P, P, P, d, S, P, P, None, P, P, None) == code, (d, S)
            assert lib.mpc_pec_supported(so, d, ops.PEC_BASIS['TABLE'], S) == 0
        assert lib.mpc_pec_supported(so, 16, ops.PEC_BASIS['TABLE'], lim // 16 - 1) & 1
        assert lib.mpc_pec_table_basis_grad(sw, P, P, P, 2, 4, P, P, None, P, P, None) == C.E_UNSUPPORTED
        # null pointers, one at a time (grad_out may be null)
        for i in (0, 1, 2, 3, 6, 7, 9, 10):
            args = [so, P, P, P, 2, 4, P, P, None, P, P, None]
            args[i] = None
            assert lib.mpc_pec_table_basis_grad(*args) == C.E_NULL, i
        for i in (0, 1, 3, 4):
            args = [P, P, None, P, P, 1, 4, 2, 2, None]
            args[i] = None
            assert lib.mpc_pec_field_basis_grad(*args) == C.E_NULL, i
        assert lib.mpc_pec_field_basis_grad(P, P, None, P, P, 1, 4, 17, 2, None) == C.E_UNSUPPORTED         # d = 17
        assert lib.mpc_pec_field_basis_grad(P, P, None, P, P, 1, 4, 2, 65, None) == C.E_UNSUPPORTED         # nbm = 65
        assert lib.mpc_pec_field_basis_grad(P, P, None, P, P, 1, 4, 0, 2, None) == C.E_SHAPE
        assert lib.mpc_pec_field_basis_grad(P, P, None, P, P, 1, 4, 2, 0, None) == C.E_SHAPE
    assert kt.summary() == {}
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), before)


@pytest.mark.parametrize('G,d,nbm', [(1, 1, 1), (255, 16, 64), (16400, 10, 5)])
def test_field_basis_gradient_against_einsum(G, d, nbm):
    """mpc_pec_field_basis_grad alone against a float64 einsum: one workgroup, a ragged one at the largest d and nbm, and more
    blocks of cells than the 64 parts (a second trip of a part's loop); bitwise equal from run to run."""
    from motionpriorcmax_amd import _lib as C
    dev = _dev()
    Bn = 2
    g = torch.Generator().manual_seed(G)
    gf = torch.randn(Bn * nbm, G, 2, generator=g)
    rows = torch.randn(Bn * G, 2 * d, generator=g)
    go = torch.tensor([0.7])
    want = 0.7 * torch.einsum('btcd,bcdj->tj', gf.double().view(Bn, nbm, G, 2), rows.double().view(Bn, G, 2, d))
    outs = []
    gf_d, rows_d, go_d = gf.to(dev), rows.to(dev), go.to(dev)
    for _ in range(2):
        part = torch.empty(nbm * 64 * d, dtype=torch.float64, device=dev)
        out = torch.full((nbm, d), float('nan'), device=dev)
        C.check(C.lib().mpc_pec_field_basis_grad(_p(gf_d), _p(rows_d), _p(go_d), _p(part), _p(out), Bn, G, d, nbm, None), 'mpc_pec_field_basis_grad')
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    # fp64 sums of exact fp32 products, one rounding to fp32 at the end (and the fp32 grad_out): 2^-23 of the sum of magnitudes
    mag = 0.7 * torch.einsum('btcd,bcdj->tj', gf.double().abs().view(Bn, nbm, G, 2), rows.double().abs().view(Bn, G, 2, d))
    assert ((outs[0].double() - want).abs() <= 2.0 ** -23 * mag + 1e-30).all()
