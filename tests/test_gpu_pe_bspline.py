"""UNPINNED extension: the cubic B-spline kind of the per-event curve warp (`FocusLoss.calc_per_event_curves(curve_type='BSPLINE')`,
csrc/pe_curves.hip: MPC_PEC_BSPLINE) against its float64 definition (tests/pe_bspline_cases.py: a Cox-de Boor of its own), bit for
bit against the unfused route through the torch mirror, at its knots, and for what the kernels skip: the orders outside the support.
(Host side: tests/test_pe_bspline_host.py.)"""
import ctypes

import pytest
import torch

import pe_bspline_cases as BC
import pe_curves_cases as PC

pytestmark = pytest.mark.gpu

KIND = 3          # include/mpcmax.h: MPC_PEC_BSPLINE


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def _loss(cfg):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _step(L, params, mask, t_ref, batch, curve='BSPLINE', fused=True, tap=False):
    """One forward + backward -> (loss, misc, grad_params, grad_mask, grad_rows or None)."""
    from motionpriorcmax_amd import ops
    dev = batch['events'].device
    pg = params.to(dev).requires_grad_(True)
    mg = mask.to(dev).requires_grad_(True) if mask is not None else None
    ops.PEC_ROWS_GRAD_TAP = [] if tap else None
    try:
        loss, log, misc = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type=curve, fused=fused)
        loss.backward()
        g_rows = ops.PEC_ROWS_GRAD_TAP[0] if tap else None
    finally:
        ops.PEC_ROWS_GRAD_TAP = None
    return loss.detach(), misc, pg.grad, mg.grad if mg is not None else None, g_rows


def _case_batch(L, name, dev):
    cfg, ev, num_pos, params, mask = BC.case_inputs(name)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if BC.CASES[name]['ordered']:
        batch = L.order_events(batch)
    return batch, params, mask


def _rel_l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize('name', list(BC.CASES))
def test_against_the_definition(name):
    """The bounds test_gpu_pe_curves.py::test_against_the_definition holds the other kinds to."""
    dev = _dev()
    c = BC.CASES[name]
    L = _loss(BC.loss_cfg(name))
    batch, params, mask = _case_batch(L, name, dev)
    ref = BC.reference(name)
    loss, misc, gp, gm, g_rows = _step(L, params, mask, c['t_ref'], batch, tap=True)
    print(f'{name}: loss {loss.item():.9g} against {ref["loss"]:.9g}')
    assert abs(loss.item() - ref['loss']) <= 1e-5 * abs(ref['loss'])
    iw = ref['iwes'].reshape(misc['iwes'].shape)
    worst = float((misc['iwes'].double().cpu() - iw).abs().max() / iw.abs().max())
    print(f'{name}: IWEs differ by {worst:.3e} of the maximum')
    assert worst <= 1e-5
    assert torch.isfinite(gp).all() and torch.isfinite(g_rows).all()
    res = BC.rows_accounting(name, g_rows.cpu(), label=name)
    print(f'{name}: row gradient accounting {res}')
    if c['norm'] == 'l2':
        r = _rel_l2(gp, ref['g_params'])
        print(f'{name}: relative L2 of grad_params {r:.3e}')
        assert r < 1e-4
        if mask is not None:
            r = _rel_l2(gm, ref['g_mask'])
            print(f'{name}: relative L2 of grad_mask {r:.3e}')
            assert r < 1e-4
    if mask is not None:
        # only the mask channels the tile centres read receive gradient (tile 4: sub-positions 2 and 6 of the 8 x 8 cell)
        g = gm.reshape(BC.B, 9, 8, 8, *gm.shape[-2:])
        off = torch.ones(8, dtype=torch.bool)
        off[[2, 6]] = False
        assert float(g[:, :, off].abs().max()) == 0.0 and float(g[:, :, :, off].abs().max()) == 0.0


def _shape_of(L, ev, num_pos):
    from motionpriorcmax_amd import ops
    return ops._pec_shape(L._cfg, ev, num_pos)


def _warp_both(sh, ev, rows, d, t_ref):
    """(mpc_pec_warp with the basis in registers, mpc_pe_warp with the dense phi [B, M, d] of the torch mirror) on the same rows."""
    from motionpriorcmax_amd import ops, utils
    dev = ev.device
    tr = torch.full((1,), t_ref, dtype=torch.float32, device=dev)
    out = torch.empty_like(ev)
    ops._call('mpc_pec_warp', dev, ctypes.byref(sh), ops._ptr(ev), ops._ptr(rows), KIND, d, None, 0, ops._ptr(tr), ops._ptr(out))
    phi = (utils.curve_event_basis(tr, d, 'BSPLINE') - utils.curve_event_basis(ev[..., 2], d, 'BSPLINE')).contiguous()
    out_m = torch.empty_like(ev)
    ops._call('mpc_pe_warp', dev, ctypes.byref(sh), ops._ptr(ev), ops._ptr(rows), ops._ptr(phi), d, ops._ptr(tr), ops._ptr(out_m))
    return out, out_m


@pytest.mark.parametrize('name', ['bspline3', 'bspline5', 'bspline10', 'bspline16'])
def test_fused_equals_the_unfused_composition_bit_for_bit(name):
    """Head rows, warped rows (as int32 patterns) and IWEs of fused=True equal fused=False: the basis in registers is the mirror's
    lines, and the coefficient pairs the warp does not read would have added c * 0."""
    from motionpriorcmax_amd import ops, utils
    dev = _dev()
    c = BC.CASES[name]
    cfg, ev, num_pos, params, mask = BC.case_inputs(name)
    L = _loss(cfg)
    ev, params = ev.to(dev), params.to(dev)
    mask = mask.to(dev) if mask is not None else None
    d = c['d']
    sh = _shape_of(L, ev, num_pos)
    rows = torch.empty(sh.B * sh.hq * sh.wq, 2 * d, device=dev)
    ops._call('mpc_pec_head_rows', dev, ops._ptr(params), ops._ptr(mask), 1.0, 4, ops._ptr(rows), sh.B, d, params.shape[2], params.shape[3])
    rows_m = utils.curve_head_rows(params, mask, 1.0, 4).contiguous()
    assert torch.equal(rows, rows_m)
    out, out_m = _warp_both(sh, ev, rows, d, c['t_ref'])
    print(f'{name}: warped rows differ in {int((out.view(torch.int32) != out_m.view(torch.int32)).sum())} of {out.numel()} elements')
    assert torch.equal(out.view(torch.int32), out_m.view(torch.int32))          # (bit patterns: column 4 holds the cell index)
    assert float((out[..., :2] - ev[..., :2]).abs().max()) > 0
    batch = {'events': ev, 'num_pos_events': num_pos}
    with torch.no_grad():
        la, _, ma = L.calc_per_event_curves(params, c['t_ref'], batch, up_mask=mask, curve_type='BSPLINE')
        lb, _, mb = L.calc_per_event_curves(params, c['t_ref'], batch, up_mask=mask, curve_type='BSPLINE', fused=False)
    assert torch.equal(ma['iwes'], mb['iwes'])
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))          # (the smoothness field of the unfused route is a GEMM)


def knot_batch(d, shape=(16, 24), sp=4, per_time=6):
    """A tiny batch (CPU tensors) whose event times are 0, 1, every knot k / L and its two fp32 neighbours, each at `per_time`
    positions and in both polarities, and tile rows of ~N(0, 4^2) pixels."""
    t = BC.knot_times(d).repeat_interleave(per_time)
    M = 2 * t.numel()
    ev, num_pos = PC.O.synth_events(1, M, shape, PC.NB, seed=17 + d)
    ev[0, :, 2] = torch.cat((t, t))
    ev[..., 4] = torch.clamp(torch.floor(ev[..., 2].clamp(0, 1) * PC.NB), 0, PC.NB - 1)
    rows = torch.randn((shape[0] // sp) * (shape[1] // sp), 2 * d, generator=torch.Generator().manual_seed(d)) * 4.0
    return PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=sp), ev, num_pos, rows


def knot_want(ev, rows, cell, d, t_ref):
    """float64: (warped (y, x) [M, 2], the bound per coordinate [M, 2] = the basis bound at degree d x sum_j |c_j|)."""
    c = rows.double().reshape(-1, 2, d)[cell]                                                     # [M, 2, d]
    phi = BC.bspline64(torch.tensor([t_ref], dtype=torch.float32), d) - BC.bspline64(ev[0, :, 2], d)          # [M, d]
    want = ev[0, :, :2].double() + (c * phi[:, None, :]).sum(-1)
    return want, BC.basis_bound_of_degree(d) * c.abs().sum(-1)


@pytest.mark.parametrize('d', [5, 10])
def test_knot_times(d):
    """mpc_pec_warp at t = 0, 1, every knot and its fp32 neighbours (d = 5: 1/3 and 2/3 are not fp32 numbers, the rounding of x
    picks the span), with t_ref off and on a knot: bit-equal to the mirror route, and every warped coordinate within (basis bound) x
    sum_j |c_j| of float64."""
    dev = _dev()
    cfg, ev, num_pos, rows = knot_batch(d)
    L = _loss(cfg)
    evd, rowsd = ev.to(dev), rows.to(dev)
    sh = _shape_of(L, evd, num_pos)
    L_spans = d - 2
    for t_ref in (0.41, float(torch.tensor(1.0 / L_spans, dtype=torch.float32)), 1.0):
        out, out_m = _warp_both(sh, evd, rowsd, d, t_ref)
        assert torch.equal(out.view(torch.int32), out_m.view(torch.int32)), t_ref
        cell = out[0, :, 4].contiguous().view(torch.int32).long().cpu()
        want, bound = knot_want(ev, rows, cell, d, t_ref)
        err = (out[0, :, :2].double().cpu() - want).abs()
        print(f'd={d} t_ref={t_ref:.7g}: worst warped error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}')
        assert (err <= bound).all()
    # the end points are exact: with t_ref = 0 an event at t = 0 does not move at all, one at t = 1 moves by minus the last control point
    out, _ = _warp_both(sh, evd, rowsd, d, 0.0)
    t0, t1 = (evd[0, :, 2] == 0.0), (evd[0, :, 2] == 1.0)
    assert int(t0.sum()) >= 12 and int(t1.sum()) >= 12
    assert torch.equal(out[0, t0, :2], evd[0, t0, :2])
    cell = out[0, t1, 4].contiguous().view(torch.int32).long()
    assert torch.equal(out[0, t1, :2], evd[0, t1, :2] + rowsd.reshape(-1, 2, d)[cell][..., d - 1] * -1.0)


def _small(dev, d, t_ref, time_scale=1.0, shape=(32, 40), M=3000, seed=4, sp=4):
    """A small image, the B-spline warp of its bucket-ordered events (times scaled by `time_scale`, the bin column left as it was: a
    caller's bins need not match its times) and a random position gradient (zero on the padding rows), for the C entry points."""
    from motionpriorcmax_amd import ops
    cfg = PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=sp)
    L = _loss(cfg)
    ev, num_pos = PC.O.synth_events(2, M, shape, PC.NB, seed=seed, pad_frac=0.1)
    ev[..., 2] *= time_scale
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(2 * (shape[0] // sp) * (shape[1] // sp), 2 * d, generator=g) * 2).to(dev)
    gpos = (torch.randn(2, M, 2, generator=g).to(dev) * (ob['events'][..., 5:6] != 0)).contiguous()
    sh = ops._pec_shape(L._cfg, ob['events'], num_pos)
    out, _ = _warp_both(sh, ob['events'], rows, d, t_ref)
    return ob, sh, out, gpos


def _rows_grad(sh, out, offs, gpos, d, opp, t_ref):
    from motionpriorcmax_amd import ops
    dev = out.device
    tr = torch.full((1,), t_ref, dtype=torch.float32, device=dev)
    dst = torch.full((sh.B * sh.hq * sh.wq, 2 * d), float('nan'), device=dev)
    ops._call('mpc_pec_rows_grad', dev, ctypes.byref(sh), ops._ptr(out), ops._ptr(offs), ops._ptr(gpos), KIND, d, None, 0, ops._ptr(tr), None,
              None, opp, ops._ptr(dst))
    return dst


@pytest.mark.parametrize('t_ref,inside', [(0.05, [0, 1, 2]), (1.0, [0, 1, 2, 9])])
def test_row_gradients_vanish_outside_the_support(t_ref, inside):
    """d = 10 (L = 8), every event in the first span (t < 1/8: s = 0, the window [s - 1, s + 2] holds the orders 0..2 of the 0-based
    ten): with t_ref in the same span the row gradients of the orders 3..9 are exactly 0.0; with t_ref = 1 (s = 7: the window is
    6..9) those outside the union of the two windows are -- and inside it only order 9 joins, E(1) being exactly one-hot -- on the
    ordered and on the atomic path.  The events' bin column is left as synthesised for times over all of [0, 1]: the kernels decide
    from each row's own time."""
    dev = _dev()
    d = 10
    ob, sh, out, gpos = _small(dev, d, t_ref, time_scale=0.12)
    assert float(out[..., 2].max()) < 0.125 and len(set(ob['events'][..., 4][ob['events'][..., 5] != 0].tolist())) > 1
    window = sorted(set(range(0, 3)) | (set(range(6, 10)) if t_ref == 1.0 else set()))
    for offs in (ob['event_offsets'], None):
        g = _rows_grad(sh, out, offs, gpos, d, 0, t_ref).reshape(-1, 2, d)
        assert torch.isfinite(g).all()
        outside = [j for j in range(d) if j not in window]
        assert float(g[..., outside].abs().max()) == 0.0
        nz = [j for j in range(d) if float(g[..., j].abs().max()) > 0]
        print(f't_ref={t_ref} {"ordered" if offs is not None else "atomic"}: orders with a gradient {nz}')
        assert nz == inside


def test_ordered_backward_is_reproducible_and_equal_across_orders_per_pass():
    """d = 10: two runs of the step on a bucket-ordered batch write the same bits, and through the C entry point 10, 4 and 1 passes
    do (integer sums per element; a skipped order would have added the integer 0), equal to a float64 index_add to the resolution
    of Q33.30."""
    from motionpriorcmax_amd import utils
    dev = _dev()
    name, d = 'bspline10', 10
    c = BC.CASES[name]
    L = _loss(BC.loss_cfg(name))
    batch, params, mask = _case_batch(L, name, dev)
    a = _step(L, params, mask, c['t_ref'], batch, tap=True)
    b = _step(L, params, mask, c['t_ref'], batch, tap=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    ob, sh, out, gpos = _small(dev, d, 0.41)
    got = [_rows_grad(sh, out, ob['event_offsets'], gpos, d, k, 0.41) for k in (1, 3, d, 0)]
    assert all(torch.equal(got[0], g) for g in got[1:])
    tr = torch.full((1,), 0.41, device=dev)
    phi = (utils.curve_event_basis(tr, d, 'BSPLINE') - utils.curve_event_basis(out[..., 2], d, 'BSPLINE')).double()
    cell = out[..., 4].contiguous().view(torch.int32).long().reshape(-1)
    contrib = (gpos.double()[:, :, :, None] * phi[:, :, None, :]).reshape(-1, 2 * d)
    want = torch.zeros(sh.B * sh.hq * sh.wq, 2 * d, dtype=torch.float64, device=dev).index_add_(0, cell, contrib)
    # Q33.30 with rounding to nearest: half a unit of 2^-30 per product, ~3000 / 80 rows per cell
    assert (got[0].double() - want).abs().max() <= 200 * 2.0 ** -31 + 1e-6 * want.abs().max()
    atomic = _rows_grad(sh, out, None, gpos, d, 0, 0.41)
    assert (atomic.double() - want).abs().max() <= 1e-5 * want.abs().max()


def test_degree_3_is_the_cubic_bezier_curve():
    """'BSPLINE' at d = 3 (one span) against 'BEZIER' at d = 3 on the same inputs: the IWEs agree within 1e-5 of the maximum."""
    dev = _dev()
    name = 'bspline3'
    c = BC.CASES[name]
    cfg, ev, num_pos, params, mask = BC.case_inputs(name)
    L = _loss(cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    with torch.no_grad():
        la, _, ma = L.calc_per_event_curves(params.to(dev), c['t_ref'], batch, curve_type='BSPLINE')
        lb, _, mb = L.calc_per_event_curves(params.to(dev), c['t_ref'], batch, curve_type='BEZIER')
    worst = float((ma['iwes'] - mb['iwes']).abs().max() / mb['iwes'].abs().max())
    print(f'BSPLINE d=3 against BEZIER d=3: IWEs differ by {worst:.3e} of the maximum, losses {float(la):.9g} {float(lb):.9g}')
    assert worst <= 1e-5


def test_the_library_refuses_fewer_than_three_control_points():
    from motionpriorcmax_amd import ops
    dev = _dev()
    cfg, ev, num_pos, *_ = BC.case_inputs('bspline3')
    L = _loss(cfg)
    evd = ev.to(dev)
    assert [ops.pec_supported(L._cfg, evd, num_pos, d, 'BSPLINE') & 1 for d in (1, 2, 3, 16, 17)] == [0, 0, 1, 1, 0]
    sh = _shape_of(L, evd, num_pos)
    rows = torch.zeros(sh.B * sh.hq * sh.wq, 4, device=dev)
    tr = torch.zeros(1, device=dev)
    with pytest.raises(Exception, match='degree >= 3'):
        ops._call('mpc_pec_warp', dev, ctypes.byref(sh), ops._ptr(evd), ops._ptr(rows), KIND, 2, None, 0, ops._ptr(tr), ops._ptr(torch.empty_like(evd)))


def test_the_step_does_not_synchronise():
    dev = _dev()
    name = 'bspline10'
    c = BC.CASES[name]
    L = _loss(BC.loss_cfg(name))
    batch, params, mask = _case_batch(L, name, dev)
    pg, mg = params.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True)
    t_ref = torch.tensor([c['t_ref']], device=dev)
    L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type='BSPLINE')[0].backward()          # (first call: module loading, the bin mid-times upload)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss, _, _ = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type='BSPLINE')
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(loss).item() and torch.isfinite(pg.grad).all()
