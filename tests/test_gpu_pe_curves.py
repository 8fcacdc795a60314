"""UNPINNED extension: the per-event continuous-time warp along RAFT-spline curves (`FocusLoss.calc_per_event_curves`,
csrc/pe_curves.hip) against its float64 definition (tests/pe_curves_cases.py), bit for bit against the routes that existed before
it, and at its edges.  (Host side: tests/test_pe_curves_host.py.)"""
import ctypes

import pytest
import torch

import pe_curves_cases as PC

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def _loss(cfg):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _step(L, params, mask, t_ref, batch, curve, table, scale=1.0, fused=True, tap=False):
    """One forward + backward -> (loss, misc, grad_params, grad_mask, grad_rows or None)."""
    from motionpriorcmax_amd import ops
    dev = batch['events'].device
    pg = params.to(dev).requires_grad_(True)
    mg = mask.to(dev).requires_grad_(True) if mask is not None else None
    ops.PEC_ROWS_GRAD_TAP = [] if tap else None
    try:
        loss, log, misc = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg, curve_type=curve,
                                                  basis_table=table.to(dev) if table is not None else None, scale=scale, fused=fused)
        loss.backward()
        g_rows = ops.PEC_ROWS_GRAD_TAP[0] if tap else None
    finally:
        ops.PEC_ROWS_GRAD_TAP = None
    return loss.detach(), misc, pg.grad, mg.grad if mg is not None else None, g_rows


def _case_batch(L, name, dev):
    cfg, ev, num_pos, params, mask, table = PC.case_inputs(name)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if PC.CASES[name]['ordered']:
        batch = L.order_events(batch)
    return batch, params, mask, table


def _rel_l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize('name', list(PC.CASES))
def test_against_the_definition(name):
    dev = _dev()
    c = PC.CASES[name]
    cfg = PC.case_inputs(name)[0]
    L = _loss(cfg)
    batch, params, mask, table = _case_batch(L, name, dev)
    ref = PC.reference(name)
    loss, misc, gp, gm, g_rows = _step(L, params, mask, c['t_ref'], batch, c['curve'], table, tap=True)
    print(f'{name}: loss {loss.item():.9g} against {ref["loss"]:.9g}')
    assert abs(loss.item() - ref['loss']) <= 1e-5 * abs(ref['loss'])
    iw = ref['iwes'].reshape(misc['iwes'].shape)
    assert (misc['iwes'].double().cpu() - iw).abs().max() <= 1e-5 * iw.abs().max()
    assert torch.isfinite(gp).all() and torch.isfinite(g_rows).all()
    PC.rows_accounting(name, g_rows.cpu(), label=name)
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
        g = gm.reshape(PC.B, 9, 8, 8, *gm.shape[-2:])
        off = torch.ones(8, dtype=torch.bool)
        off[[2, 6]] = False
        assert float(g[:, :, off].abs().max()) == 0.0 and float(g[:, :, :, off].abs().max()) == 0.0


def _c_rows_and_warp(L, ev, num_pos, params, mask, t_ref, curve, table, scale, tile):
    """Through the C entry points: (head rows, warped rows) of the curve kernels, and of the route a caller could already run --
    rows from the plain-torch mirror, phi [B, M, d] from utils.curve_event_basis, mpc_pe_warp."""
    from motionpriorcmax_amd import ops, utils
    dev = ev.device
    Bn, M, _ = ev.shape
    d = params.shape[1] // 2
    sh = ops._pec_shape(L._cfg, ev, num_pos)
    G = sh.hq * sh.wq
    tr = torch.full((1,), t_ref, dtype=torch.float32, device=dev)
    rows = torch.empty(Bn * G, 2 * d, device=dev)
    ops._call('mpc_pec_head_rows', dev, ops._ptr(params), ops._ptr(mask), float(scale), tile, ops._ptr(rows), Bn, d, params.shape[2], params.shape[3])
    out = torch.empty_like(ev)
    S = table.shape[0] - 1 if table is not None else 0
    ops._call('mpc_pec_warp', dev, ctypes.byref(sh), ops._ptr(ev), ops._ptr(rows), ops.PEC_BASIS[curve], d, ops._ptr(table), S, ops._ptr(tr), ops._ptr(out))
    rows_m = utils.curve_head_rows(params, mask, scale, tile).contiguous()
    phi = (utils.curve_event_basis(tr, d, curve, table) - utils.curve_event_basis(ev[..., 2], d, curve, table)).contiguous()
    out_m = torch.empty_like(ev)
    ops._call('mpc_pe_warp', dev, ctypes.byref(sh), ops._ptr(ev), ops._ptr(rows_m), ops._ptr(phi), d, ops._ptr(tr), ops._ptr(out_m))
    return rows, out, rows_m, out_m


@pytest.mark.parametrize('name', ['bezier10', 'bezier16', 'polynomial3', 'polynomial9', 'bspline8', 'bezier1'])
def test_fused_equals_the_unfused_composition_bit_for_bit(name):
    """Head rows, warped rows and IWEs of fused=True equal fused=False: the basis in registers is the mirror's lines, the head
    rows the mirror's sums."""
    dev = _dev()
    c = PC.CASES[name]
    cfg, ev, num_pos, params, mask, table = PC.case_inputs(name)
    L = _loss(cfg)
    ev, params = ev.to(dev), params.to(dev)
    mask = mask.to(dev) if mask is not None else None
    table = table.to(dev) if table is not None else None
    rows, out, rows_m, out_m = _c_rows_and_warp(L, ev, num_pos, params, mask, c['t_ref'], c['curve'], table, 1.0, 4)
    print(f'{name}: head rows differ in {int((rows != rows_m).sum())} of {rows.numel()} elements, warped rows in '
          f'{int((out.view(torch.int32) != out_m.view(torch.int32)).sum())}')
    assert torch.equal(rows, rows_m)
    assert torch.equal(out.view(torch.int32), out_m.view(torch.int32))          # (bit patterns: column 4 holds the cell index)
    batch = {'events': ev, 'num_pos_events': num_pos}
    with torch.no_grad():
        la, _, ma = L.calc_per_event_curves(params, c['t_ref'], batch, up_mask=mask, curve_type=c['curve'], basis_table=table)
        lb, _, mb = L.calc_per_event_curves(params, c['t_ref'], batch, up_mask=mask, curve_type=c['curve'], basis_table=table, fused=False)
    assert torch.equal(ma['iwes'], mb['iwes'])
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))          # (the smoothness field of the unfused route is a GEMM)


@pytest.mark.parametrize('d', [3, 8])
def test_polynomial_curves_equal_the_per_event_basis_warp_bit_for_bit(d):
    """POLYNOMIAL d <= 8 through the new node against calc_per_event_basis(basis_type='polynomial') on a coefficient grid that
    holds the same rows: loss and IWEs bit for bit, the gradient to rounding."""
    dev = _dev()
    cfg = PC.loss_cfg('l1')
    L = _loss(cfg)
    ev, num_pos = PC.O.synth_events(PC.B, PC.M, PC.SHAPE, PC.NB, seed=7, pad_frac=0.1)
    batch = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    params = (torch.randn(PC.B, 2 * d, PC.HQ, PC.WQ, generator=torch.Generator().manual_seed(d)) * 3).to(dev)
    grid = torch.zeros(PC.B, 1, 2 * d, *PC.SHAPE, device=dev)
    grid[:, 0, :, PC.SP // 2::PC.SP, PC.SP // 2::PC.SP] = torch.cat((params[:, d:], params[:, :d]), dim=1)
    grid.requires_grad_(True)
    lb, _, mb = L.calc_per_event_basis(grid, 0.41, batch, d, 'polynomial')
    lb.backward()
    la, ma, gp, _, _ = _step(L, params, None, 0.41, batch, 'POLYNOMIAL', None)
    assert torch.equal(la, lb.detach()) and torch.equal(ma['iwes'], mb['iwes'])
    # (the gradient: the same products, but mpc_pe_grad_ordered rounds 16 partial sums per strip to fp32 before it adds them, the
    # curve kernel one integer sum per element -- equal to fp32 rounding, not bit for bit)
    want = grid.grad[:, 0, :, PC.SP // 2::PC.SP, PC.SP // 2::PC.SP]
    want = torch.cat((want[:, d:], want[:, :d]), dim=1)
    assert (gp - want).abs().max() <= 1e-5 * want.abs().max()


@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('k', [1, 3, 5])
def test_table_curves_equal_the_table_basis_warp_bit_for_bit(k, S):
    """TABLE curves against the tabulated basis warp through the C entry points, on the same bucket-ordered events, tile rows,
    table and t_ref: both families interpolate the table with pe_tab_locate / pe_tab_lerp and accumulate with pe_to_fixed
    (csrc/pe_device.h), so the warped rows and the tile gradients agree bit for bit.  k: one per KB instantiation of the basis
    kernels; the event times include 0, 1, every knot i / S and one value just below a knot.  The gradients: mpc_pec_rows_grad
    on the position gradient that mpc_pe_table_grad_ordered (split = 1, grad_out = 1) leaves behind from the same adjoint image."""
    from motionpriorcmax_amd import _lib as C, ops
    dev = _dev()
    shape, sp, Bn, M = (16, 24), 4, 2, 400
    L = _loss(PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=sp))
    ev, num_pos = PC.O.synth_events(Bn, M, shape, PC.NB, seed=13, pad_frac=0.1)
    knots = [i / S for i in range(S + 1)]
    below = float(torch.nextafter(torch.tensor(knots[-1] if S == 1 else knots[S // 2]), torch.tensor(0.0)))
    for blk in (0, num_pos):                                      # (both polarities)
        for i, t in enumerate(knots + [below]):
            ev[:, blk + 3 * i, 2] = t
    ev[..., 4] = torch.clamp(torch.floor(ev[..., 2] * PC.NB), 0, PC.NB - 1) * ev[..., 5]
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    evd, offs = ob['events'], ob['event_offsets']
    times = set(evd[..., 2][evd[..., 5] != 0].tolist())
    assert {0.0, 1.0, below} | set(float(torch.tensor(t, dtype=torch.float32)) for t in knots) <= times
    sh = ops._pec_shape(L._cfg, evd, num_pos)
    assert ops._query('mpc_pe_grad_ordered_supported', dev, ctypes.byref(sh), k) == 1 and ops._lut_strips(sh, dev) >= 1
    n = sh.B * sh.hq * sh.wq
    g = torch.Generator().manual_seed(100 * k + S)
    rows = (torch.randn(n, 2 * k, generator=g) * 3).to(dev)
    table = torch.randn(S + 1, k, generator=g).to(dev)
    tr = torch.full((1,), 0.41, dtype=torch.float32, device=dev)
    out_c, out_t = torch.empty_like(evd), torch.empty_like(evd)
    ops._call('mpc_pec_warp', dev, ctypes.byref(sh), ops._ptr(evd), ops._ptr(rows), ops.PEC_BASIS['TABLE'], k, ops._ptr(table), S, ops._ptr(tr),
              ops._ptr(out_c))
    ops._call('mpc_pe_table_warp', dev, ctypes.byref(sh), ops._ptr(evd), ops._ptr(rows), ops._ptr(table), S, k, ops._ptr(tr), ops._ptr(out_t))
    print(f'k={k} S={S}: warped rows differ in {int((out_c.view(torch.int32) != out_t.view(torch.int32)).sum())} of {out_c.numel()} elements')
    assert torch.equal(out_c.view(torch.int32), out_t.view(torch.int32))          # (bit patterns: column 4 holds the cell index)
    assert float((out_t[..., :2] - evd[..., :2]).abs().max()) > 0
    # the gradients, from one adjoint image (two polarity planes per sample)
    gimg = torch.randn(Bn * 2, *shape, generator=g).to(dev)
    scal = torch.ones(C.SCAL_COUNT, dtype=torch.float32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    g_t = torch.empty(1, n, 2 * k, device=dev)
    gpos = torch.empty(Bn, M, 2, device=dev)
    ops._call('mpc_pe_table_grad_ordered', dev, ctypes.byref(sh), ops._ptr(out_t), ops._ptr(offs), ops._ptr(table), S, k, ops._ptr(tr), ops._ptr(gimg),
              ops._ptr(scal), ops._ptr(one), ops._ptr(g_t), 1, ops._ptr(gpos))
    g_c = torch.empty(n, 2 * k, device=dev)
    ops._call('mpc_pec_rows_grad', dev, ctypes.byref(sh), ops._ptr(out_c), ops._ptr(offs), ops._ptr(gpos), ops.PEC_BASIS['TABLE'], k, ops._ptr(table), S,
              ops._ptr(tr), ops._ptr(scal), ops._ptr(one), 0, ops._ptr(g_c))
    print(f'k={k} S={S}: tile gradients differ in {int((g_c != g_t[0]).sum())} of {g_c.numel()} elements, '
          f'largest |difference| {float((g_c - g_t[0]).abs().max()):.3e} of {float(g_t.abs().max()):.3e}')
    assert float(g_t.abs().max()) > 0 and int((gpos != 0).any(-1).sum()) > M // 2
    assert torch.equal(g_c, g_t[0])


def test_ordered_backward_is_reproducible():
    dev = _dev()
    name = 'bezier10'
    c = PC.CASES[name]
    L = _loss(PC.case_inputs(name)[0])
    batch, params, mask, table = _case_batch(L, name, dev)
    a = _step(L, params, mask, c['t_ref'], batch, c['curve'], table, tap=True)
    b = _step(L, params, mask, c['t_ref'], batch, c['curve'], table, tap=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def _small(dev, d=10, shape=(32, 40), M=3000, seed=4, sp=4, yscale=1.0):
    """A small image, the rows of the curve warp on its bucket-ordered events and a random position gradient (zero on the padding
    rows), for the C entry points."""
    from motionpriorcmax_amd import ops
    cfg = PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=sp)
    L = _loss(cfg)
    ev, num_pos = PC.O.synth_events(2, M, shape, PC.NB, seed=seed, pad_frac=0.1)
    ev[..., 0] *= yscale
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    g = torch.Generator().manual_seed(seed)
    params = (torch.randn(2, 2 * d, -(-shape[0] // sp), -(-shape[1] // sp), generator=g) * 2).to(dev)
    gpos = (torch.randn(2, M, 2, generator=g).to(dev) * (ob['events'][..., 5:6] != 0)).contiguous()
    rows, out, _, _ = _c_rows_and_warp(L, ob['events'], num_pos, params, None, 0.41, 'BEZIER', None, 1.0, sp)
    sh = ops._pec_shape(L._cfg, ob['events'], num_pos)
    return L, ob, sh, rows, out, gpos


def _rows_grad(sh, out, offs, gpos, d, opp, dst=None, go=None):
    from motionpriorcmax_amd import ops
    dev = out.device
    tr = torch.full((1,), 0.41, dtype=torch.float32, device=dev)
    if dst is None:
        dst = torch.empty(sh.B * sh.hq * sh.wq, 2 * d, device=dev)
    ops._call('mpc_pec_rows_grad', dev, ctypes.byref(sh), ops._ptr(out), ops._ptr(offs), ops._ptr(gpos), 0, d, None, 0, ops._ptr(tr), None,
              ops._ptr(go), opp, ops._ptr(dst))
    return dst


def test_ordered_row_gradient_is_equal_across_orders_per_pass():
    """d = 10 on a 32 x 40 image through the C entry point: 10, 4 and 1 passes write the same bits (integer sums per element), and
    they are the sums a float64 index_add gives; the atomic route agrees to rounding."""
    from motionpriorcmax_amd import _lib as C, utils
    dev = _dev()
    d = 10
    L, ob, sh, rows, out, gpos = _small(dev, d)
    lib = C.lib()
    assert [int(lib.mpc_pec_rows_grad_passes(ctypes.byref(sh), d, k)) for k in (1, 3, d)] == [10, 4, 1]
    assert 1 <= int(lib.mpc_pec_rows_grad_passes(ctypes.byref(sh), d, 0)) <= 10          # (the library's choice follows the CU count)
    got = [_rows_grad(sh, out, ob['event_offsets'], gpos, d, k) for k in (1, 3, d, 0)]
    assert all(torch.equal(got[0], g) for g in got[1:])
    tr = torch.full((1,), 0.41, device=dev)
    phi = (utils.curve_event_basis(tr, d, 'BEZIER') - utils.curve_event_basis(out[..., 2], d, 'BEZIER')).double()
    cell = out[..., 4].contiguous().view(torch.int32).long().reshape(-1)
    contrib = (gpos.double()[:, :, :, None] * phi[:, :, None, :]).reshape(-1, 2 * d)
    want = torch.zeros(sh.B * sh.hq * sh.wq, 2 * d, dtype=torch.float64, device=dev).index_add_(0, cell, contrib)
    # Q33.30 with rounding to nearest: half a unit of 2^-30 per product, ~3000 / 80 rows per cell
    assert (got[0].double() - want).abs().max() <= 200 * 2.0 ** -31 + 1e-6 * want.abs().max()
    atomic = _rows_grad(sh, out, None, gpos, d, 0)
    assert (atomic.double() - want).abs().max() <= 1e-5 * want.abs().max()
    # a loss scale is applied after the sums
    go = torch.full((1,), 8.0, device=dev)
    assert torch.equal(_rows_grad(sh, out, ob['event_offsets'], gpos, d, 3, go=go), 8.0 * got[0])


def test_scaled_events_against_the_definition():
    """Net 32 x 32 (h = w = 4), events 40 x 40, scale 1.25, sp 5: tile 4, 8 x 8 tiles = 8 x 8 look-up-table cells."""
    dev = _dev()
    shape, d, M = (40, 40), 3, 3000
    cfg = PC.loss_cfg('l2', image_shape=shape, lut_superpixel_size=5)
    ev, num_pos = PC.O.synth_events(2, M, shape, PC.NB, seed=9, pad_frac=0.1)
    g = torch.Generator().manual_seed(2)
    params, mask = torch.randn(2, 2 * d, 4, 4, generator=g) * 0.4, torch.randn(2, 576, 4, 4, generator=g)
    r = PC.definition(cfg, ev, num_pos, params, mask, 0.41, 'BEZIER', scale=1.25)
    r['loss'].backward()
    L = _loss(cfg)
    batch = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    loss, misc, gp, gm, _ = _step(L, params, mask, 0.41, batch, 'BEZIER', None, scale=1.25)
    assert abs(loss.item() - float(r['loss'].detach())) <= 1e-5 * abs(float(r['loss'].detach()))
    iw = r['iwes'].reshape(misc['iwes'].shape)
    assert (misc['iwes'].double().cpu() - iw).abs().max() <= 1e-5 * iw.abs().max()
    assert _rel_l2(gp, r['params'].grad) < 1e-4 and _rel_l2(gm, r['mask'].grad) < 1e-4


def test_zero_control_points_are_the_identity_warp_and_end_point_times_are_exact():
    from motionpriorcmax_amd import ops
    dev = _dev()
    cfg = PC.loss_cfg('l1', smooth_weight=0.0)
    L = _loss(cfg)
    ev, num_pos = PC.O.synth_events(PC.B, 9000, PC.SHAPE, PC.NB, seed=5)
    ev[:, ::7, 2] = 0.0
    ev[:, 3::7, 2] = 1.0
    evd = ev.to(dev)
    batch = {'events': evd, 'num_pos_events': num_pos}
    z = torch.zeros(PC.B, 20, PC.HQ, PC.WQ, device=dev)
    l0, _, m0 = L.calc_per_event_curves(z, 0.3, batch)
    lut = torch.zeros(PC.B, PC.NB, PC.HQ, PC.WQ, 1, 2, device=dev)
    f, iw, _ = ops.EventFocusFn.apply(lut, evd, torch.tensor([0.3], device=dev), L._cfg, num_pos)
    assert torch.equal(l0, f) and torch.equal(m0['iwes'].reshape(iw.shape), iw)
    # Bezier curves: E(0) = 0 and E(1) = one-hot exactly, so with t_ref = 0 the events at t = 0 stay where they are, bit for bit,
    # and those at t = 1 move by exactly minus the last control point
    p = (torch.randn(PC.B, 20, PC.HQ, PC.WQ, generator=torch.Generator().manual_seed(1)) * 3).to(dev)
    rows, out, _, out_m = _c_rows_and_warp(L, evd, num_pos, p, None, 0.0, 'BEZIER', None, 1.0, 4)
    assert torch.equal(out.view(torch.int32), out_m.view(torch.int32))
    assert torch.equal(out[:, ::7, :2], evd[:, ::7, :2])
    cell = out[:, 3::7, 4].contiguous().view(torch.int32).long()
    last = rows.reshape(-1, 2, 10)[cell][..., 9]                                  # [B, m, 2]
    assert torch.equal(out[:, 3::7, :2], evd[:, 3::7, :2] + last * -1.0)
    # ... and the whole step agrees with the definition there
    cfg2 = PC.loss_cfg('l2')
    r = PC.definition(cfg2, ev, num_pos, p.cpu(), None, 1.0, 'BEZIER')
    l1, _, _ = _loss(cfg2).calc_per_event_curves(p, 1.0, batch)
    assert abs(l1.item() - float(r['loss'].detach())) <= 1e-5 * abs(float(r['loss'].detach()))


def test_a_strip_without_events_no_events_at_all_and_a_wrong_tile_count():
    from motionpriorcmax_amd import ops
    dev = _dev()
    d = 10
    # 200 x 128 at sp = 2: 100 x 64 cells in three strips of 34 rows (48 KB / (64 * 16) = 48 rows at most); the events lie in the
    # top 40 pixels, so the second and third strip hold none
    L, ob, sh, rows, out, gpos = _small(dev, d, shape=(200, 128), M=3000, sp=2, yscale=0.2)
    assert ops._lut_strips(sh, dev) >= 2
    got = _rows_grad(sh, out, ob['event_offsets'], gpos, d, 0)
    atomic = _rows_grad(sh, out, None, gpos, d, 0)
    assert (got - atomic).abs().max() <= 1e-5 * atomic.abs().max() and float(atomic.abs().max()) > 0
    assert float(got.reshape(2, 100, 64, -1)[:, 34:].abs().max()) == 0.0
    # M = 0: empty images; the step runs both ways and no event moves the control points
    L2 = _loss(PC.loss_cfg('l2'))
    empty = {'events': torch.zeros(PC.B, 0, 6, device=dev), 'num_pos_events': 0}
    p = torch.randn(PC.B, 6, PC.HQ, PC.WQ, device=dev).requires_grad_(True)
    loss, _, misc = L2.calc_per_event_curves(p, 0.41, empty)
    loss.backward()
    assert float(misc['iwes'].abs().max()) == 0.0 and torch.isfinite(p.grad).all()
    # a tile count that does not match: refused before anything is launched
    with ops.KernelTimer() as kt:
        with pytest.raises(ValueError, match='look-up-table grid'):
            L2.calc_per_event_curves(torch.zeros(PC.B, 6, PC.HQ, PC.WQ - 1, device=dev), 0.41, empty)
        with pytest.raises(ValueError, match='look-up-table grid'):
            L2.calc_per_event_curves(torch.zeros(PC.B, 6, 12, 16, device=dev), 0.41, empty, up_mask=torch.zeros(PC.B, 576, 12, 16, device=dev), scale=0.5)
    assert kt.summary() == {}


def test_guard_bands_stay_untouched():
    """NaN-patterned bands around rows, grad_rows, grad_params and grad_mask: every element inside is written, none outside."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    d, Bn, h, w, tile, pad = 5, 2, 3, 5, 4, 1024
    nty, ntx = 8 * h // tile, 8 * w // tile
    G = nty * ntx
    g = torch.Generator().manual_seed(6)
    params, mask = torch.randn(Bn, 2 * d, h, w, generator=g).to(dev), torch.randn(Bn, 576, h, w, generator=g).to(dev)

    def band(n):
        return torch.full((n + 2 * pad,), float('nan'), device=dev)

    def check(buf, n):
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n:]).all() and torch.isfinite(buf[pad:pad + n]).all()

    rows = band(Bn * G * 2 * d)
    ops._call('mpc_pec_head_rows', dev, ops._ptr(params), ops._ptr(mask), 1.0, tile, ops._ptr(rows[pad:]), Bn, d, h, w)
    check(rows, Bn * G * 2 * d)
    g_rows = torch.randn(Bn * G, 2 * d, generator=g).to(dev)
    gp, gm = band(Bn * 2 * d * h * w), band(Bn * 576 * h * w)
    nws = ops._query('mpc_pec_head_rows_bwd_workspace_bytes', dev, Bn, d, h, w, tile)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    ops._call('mpc_pec_head_rows_bwd', dev, ops._ptr(g_rows), ops._ptr(params), ops._ptr(mask), 1.0, tile, ops._ptr(gp[pad:]), ops._ptr(gm[pad:]),
              Bn, d, h, w, ops._ptr(ws))
    check(gp, Bn * 2 * d * h * w)
    check(gm, Bn * 576 * h * w)
    # the adjoint pairs with the forward: <head(p, m) rows, g> has the directional derivative <grad_params, dp> along dp
    dp = torch.randn(Bn, 2 * d, h, w, generator=g).to(dev) * 1e-2
    r0, r1 = torch.empty(Bn * G, 2 * d, device=dev), torch.empty(Bn * G, 2 * d, device=dev)
    ops._call('mpc_pec_head_rows', dev, ops._ptr(params - dp), ops._ptr(mask), 1.0, tile, ops._ptr(r0), Bn, d, h, w)
    ops._call('mpc_pec_head_rows', dev, ops._ptr((params + dp).contiguous()), ops._ptr(mask), 1.0, tile, ops._ptr(r1), Bn, d, h, w)
    lhs = float(((r1 - r0).double() * g_rows.double()).sum()) / 2
    rhs = float((gp[pad:pad + dp.numel()].reshape(dp.shape).double() * dp.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * abs(rhs)
    # without a mask
    gp2 = band(Bn * G * 2 * d)
    ops._call('mpc_pec_head_rows_bwd', dev, ops._ptr(g_rows), ops._ptr(params), None, 1.5, tile, ops._ptr(gp2[pad:]), None, Bn, d, nty, ntx, None)
    check(gp2, Bn * G * 2 * d)
    # the row gradient, ordered (several passes) and atomic
    L, ob, sh, _, out, gpos = _small(dev, 10)
    n = sh.B * sh.hq * sh.wq * 20
    for offs, opp in ((ob['event_offsets'], 3), (None, 0)):
        buf = band(n)
        _rows_grad(sh, out, offs, gpos, 10, opp, dst=buf[pad:])
        check(buf, n)


def test_the_step_does_not_synchronise():
    dev = _dev()
    name = 'bezier10'
    c = PC.CASES[name]
    L = _loss(PC.case_inputs(name)[0])
    batch, params, mask, table = _case_batch(L, name, dev)
    pg, mg = params.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True)
    t_ref = torch.tensor([c['t_ref']], device=dev)
    L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg)[0].backward()          # (first call: module loading, the bin mid-times upload)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss, _, _ = L.calc_per_event_curves(pg, t_ref, batch, up_mask=mg)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(loss).item() and torch.isfinite(pg.grad).all()
