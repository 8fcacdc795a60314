"""FocusLoss.calc_per_event_basis(basis_type='table') on the GPU: the kernels that read a tabulated motion basis and reduce the
batch's gradient onto its entries (csrc/pe_basis.hip: the TAB instantiations of k_pe_warp / k_pe_grad / k_pe_accum, k_pe_table_grad;
csrc/tiles.hip: k_field_basis_grad_*) against the DEFINITION in tests/pe_table_cases.py (the oracle's per-event path with the
table formula), fp32 and float64.  The rules are those of `_against_oracle` in tests/test_gpu_per_event.py, restated here."""
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import pe_table_cases as PT

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def _cfg(shape, nb, **over):
    cfg = dict(image_shape=shape, num_tref=1, num_bins=nb, num_knn=8, smooth_weight=0.003, lut_superpixel_size=4,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    cfg.update(over)
    return cfg


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _run(L, coeff, table, t_ref, batch, fused=True, table_fn=None):
    """One forward and backward on the device -> (loss, iwes, grad of the coefficients, grad of the table or of the parameters)."""
    dev = batch['events'].device
    cg = coeff.to(dev).requires_grad_(True)
    params = None
    if table_fn is not None:
        tb, params = table_fn(dev)
    else:
        tb = table.to(dev).requires_grad_(True)
    lg, _, mg = L.calc_per_event_basis(cg, t_ref, batch, tb.shape[1], 'table', fused=bool(fused), basis_table=tb)
    if params is not None:
        gs = torch.autograd.grad(lg, [cg] + list(params))
        return lg.detach(), mg['iwes'], gs[0], torch.cat([g.reshape(-1) for g in gs[1:]])
    lg.backward()
    return lg.detach(), mg['iwes'], cg.grad, tb.grad


def _grad_rule(label, what, dev_g, g32, g64, bound):
    """Relative L2 against the fp32 definition below `bound`; where it is not, against float64 within 4 times the fp32 definition's
    own distance from float64 (the rule of tests/test_gpu_per_event.py and tests/test_cvx_traj_host.py).  All three figures printed."""
    r32, d_dev, d_or = PT.rel(dev_g, g32), PT.rel(dev_g, g64), PT.rel(g32, g64)
    fb = not r32 < bound
    print(f'PE_TABLE | {label} | {what} | to fp32 definition {r32:.3e} | to float64 {d_dev:.3e} | definition fp32 to float64 {d_or:.3e} | '
          f'bound {bound:.0e} | {"float64 fallback" if fb else "direct"}')
    if fb:
        assert d_or >= bound and d_dev <= 4 * d_or, (label, what, r32, d_dev, d_or)


def _against_definition(cfg, ev, num_pos, coeff, table, t_ref, out, label, table_fn32=None, table_fn64=None, loss_finite=True):
    from motionpriorcmax_amd.utils import get_optical_flow_tile_mask
    lg, iw_g, gc, gt = (o.cpu() for o in out)
    l32, iw32, gc32, gt32 = PT.definition(cfg, ev, num_pos, coeff, table, t_ref, torch.float32, table_fn32)
    _, _, gc64, gt64 = PT.definition(cfg, ev, num_pos, coeff, table, t_ref, torch.float64, table_fn64)
    if loss_finite:
        assert abs(lg.item() - l32.item()) <= 1e-5 * abs(l32.item()), (label, lg.item(), l32.item())
        iw = iw32.reshape(iw_g.shape)
        assert (iw_g - iw).abs().max() <= 1e-5 * iw.abs().max(), label
    assert torch.isfinite(gc).all() and torch.isfinite(gt).all() and gt32.abs().max() > 0, label
    sign_free = cfg['focus_loss_norm'] == 'l2' or cfg.get('loss_type') == 'variance'
    bound = 1e-4 if sign_free else 2e-3
    if gc32.abs().max() > 0:
        r = PT.rel(gc, gc32)
        if sign_free:
            _grad_rule(label, 'coefficients', gc, gc32, gc64, bound)
        else:
            print(f'PE_TABLE | {label} | coefficients | to fp32 definition {r:.3e} | to float64 {PT.rel(gc, gc64):.3e} | '
                  f'definition fp32 to float64 {PT.rel(gc32, gc64):.3e} | bound {bound:.0e} | direct')
            assert r < bound, (label, r)
    _grad_rule(label, 'table', gt, gt32, gt64, bound)
    s = cfg['lut_superpixel_size']
    assert float(gc[..., ~get_optical_flow_tile_mask(cfg['image_shape'], s)].abs().max()) == 0.0


KS, SS, FUSED = (1, 3, 8), (1, 37, 1024), (True, 'ordered', False)
OBJ = ({'focus_loss_norm': 'l1'}, {'focus_loss_norm': 'l2'}, {'loss_type': 'variance'})


def _matrix():
    """Every (k, S, fused); the objective, the smoothness term and the polarity split cycle over them so that each objective meets
    every k, every S and every route, and each of the 12 (objective, smoothness, polarity) settings occurs."""
    cases = []
    for (ik, k), (js, S), (jf, fused) in itertools.product(enumerate(KS), enumerate(SS), enumerate(FUSED)):
        o = (ik + js + jf) % 3
        smooth = (ik + 2 * js + jf + (ik * js) % 2) % 2 == 0
        pol = (js + jf + o) % 2 == 0
        cases.append(pytest.param(k, S, fused, o, smooth, pol, id=f'k{k}-S{S}-{fused}-{("l1", "l2", "var")[o]}-{"smooth" if smooth else "nosmooth"}-{"pol" if pol else "nopol"}'))
    # the settings the cycle leaves out
    seen = {(c.values[3], c.values[4], c.values[5]) for c in cases}
    for o, smooth, pol in itertools.product(range(3), (True, False), (True, False)):
        if (o, smooth, pol) not in seen:
            cases.append(pytest.param(3, 37, True, o, smooth, pol, id=f'k3-S37-True-{("l1", "l2", "var")[o]}-{"smooth" if smooth else "nosmooth"}-{"pol" if pol else "nopol"}-extra'))
    return cases


@pytest.mark.parametrize('k,S,fused,o,smooth,pol', _matrix())
def test_table_basis_against_its_definition(k, S, fused, o, smooth, pol):
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb = (96, 128), 2, 12000, 5
    cfg = _cfg(shape, nb, smooth_weight=0.003 if smooth else 0.0, polarity_aware_batching=pol, **OBJ[o])
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=11, pad_frac=0.1)
    g = torch.Generator().manual_seed(3)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0          # some events leave the image
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    ev_def = ev
    if fused == 'ordered':
        bg = L.order_events(bg)
        assert 'event_offsets' in bg
    out = _run(L, coeff, table, 0.41, bg, fused)
    _against_definition(cfg, ev_def, num_pos, coeff, table, 0.41, out, f'k={k} S={S} fused={fused} {OBJ[o]} smooth={smooth} pol={pol}')


def test_identity_table_is_the_first_order_polynomial_bit_for_bit():
    """T[i] = i / 1024 interpolates to t exactly (tests/test_pe_table_host.py), so phi is the polynomial route's t_ref - t in every
    bit, and both backward routes accumulate the same products in integers: loss, IWEs and coefficient gradient are bitwise equal."""
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb = (96, 128), 2, 12000, 5
    cfg = _cfg(shape, nb)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=12, pad_frac=0.1)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    coeff = torch.randn(B, 1, 2, *shape, generator=torch.Generator().manual_seed(5)) * 4.0
    T = (torch.arange(1025, dtype=torch.float32) / 1024)[:, None]
    lt, it, gt, _ = _run(L, coeff, T, 0.41, ob)
    cg = coeff.to(dev).requires_grad_(True)
    lp, _, mp = L.calc_per_event_basis(cg, 0.41, ob, 1, 'polynomial')
    lp.backward()
    assert torch.equal(lt, lp.detach()) and torch.equal(it, mp['iwes']) and torch.equal(gt, cg.grad)
    assert float(cg.grad.abs().max()) > 0


def _mlp(k, seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(),
                         nn.Linear(64, k))


def test_the_learned_basis_trains_through_the_per_event_warp():
    """The reference's basis network (1 -> 64 -> 64 -> 64 -> 3, LeakyReLU) sampled at 257 knots: loss.backward() reaches every
    parameter, and the parameter gradient matches the definition run end to end on the CPU."""
    from motionpriorcmax_amd import LossFactory
    from motionpriorcmax_amd.utils import basis_table
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (96, 128), 2, 12000, 5, 3, 256
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=13, pad_frac=0.1)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(6)) * 4.0
    net = _mlp(k)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}

    def on_device(d):
        n = _mlp(k).to(d)
        n.load_state_dict(net.state_dict())
        return basis_table('learned', k, S, n), list(n.parameters())

    def on_host(dtype):
        n = _mlp(k).to(dtype)
        n.load_state_dict(net.state_dict())
        knots = torch.arange(S + 1, dtype=torch.float32).to(dtype) / S
        return n(knots[:, None]), list(n.parameters())
    out = _run(L, coeff, None, 0.41, bg, table_fn=on_device)
    sizes = [p.numel() for p in net.parameters()]
    for gpart in torch.split(out[3].cpu(), sizes):
        assert torch.isfinite(gpart).all() and float(gpart.abs().max()) > 0
    _against_definition(cfg, ev, num_pos, coeff, None, 0.41, out, 'learned basis, S=256', on_host, on_host)


@pytest.mark.parametrize('S', [1, 16])
@pytest.mark.parametrize('ordered', [False, True])
def test_edges_of_the_interpolation(S, ordered):
    """Blocks of events with t exactly 0, exactly 1, exactly on knots and one ulp below knots; t_ref at 0, at 1, on a knot and inside
    the interval that holds a block of 500 events.  S = 1 puts every event into one interval (the worst case for the LDS adds)."""
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k = (96, 128), 2, 12000, 5, 3
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=14, pad_frac=0.1)
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
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if ordered:
        bg = L.order_events(bg)
    for t_ref in (0.0, 1.0, float(knots[min(1, S)]), 0.5 / S):
        out = _run(L, coeff, table, t_ref, bg)
        _against_definition(cfg, ev, num_pos, coeff, table, t_ref, out, f'edges S={S} ordered={ordered} t_ref={t_ref}')


@pytest.mark.parametrize('ordered', [False, True])
def test_rows_without_weight_contribute_exactly_nothing(ordered):
    """Rows with valid == 0 and rows that the border mask zeroes: their times change between two runs, the table gradient does not
    change in any bit."""
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (96, 128), 2, 12000, 5, 3, 37
    cfg = _cfg(shape, nb)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=15, pad_frac=0.1)
    dead = (ev[..., 5] == 0)
    assert int(dead.sum()) > 0
    far = torch.zeros(B, M, dtype=torch.bool)
    far[:, 100:400] = True
    far[:, num_pos + 100:num_pos + 400] = True
    ev[..., 0][far] = -300.0                    # far outside the image for any warp of these coefficients: masked by the border
    g = torch.Generator().manual_seed(8)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    grads = []
    for flip in (False, True):
        e = ev.clone()
        if flip:
            e[..., 2][dead | far] = 1.0 - e[..., 2][dead | far]
        bg = {'events': e.to(dev), 'num_pos_events': num_pos}
        if ordered:
            # (the layout is that of the unflipped batch for both runs: the time bins of the rows, column 4, are left alone)
            bg = L.order_events(bg)
        grads.append(_run(L, coeff, table, 0.41, bg)[3])
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_table_gradient_is_reproducible_in_every_layout():
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (96, 128), 2, 12000, 5, 3, 1024
    cfg = _cfg(shape, nb)
    g = torch.Generator().manual_seed(9)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    for time_sorted in (True, False):
        ev, num_pos = O.synth_events(B, M, shape, nb, seed=16, pad_frac=0.1, time_sorted=time_sorted)
        bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
        a, b = _run(L, coeff, table, 0.41, bg)[3], _run(L, coeff, table, 0.41, bg)[3]
        assert torch.equal(a, b) and float(a.abs().max()) > 0, time_sorted
        ob = L.order_events(bg)
        c, d = _run(L, coeff, table, 0.41, ob)[3], _run(L, coeff, table, 0.41, ob)[3]
        assert torch.equal(c, d), time_sorted
        # the same events in the other layout: the same per-event products, summed in integers
        assert torch.equal(a, c), time_sorted


def test_second_trip_of_the_table_gradient_kernel():
    """k_pe_table_grad runs at most 256 workgroups of 1024 rows: B * M = 262 202 rows is more than 262 144 and no multiple of 1024,
    so the first workgroups make a second trip and the last one is ragged."""
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (16, 24), 2, 131101, 3, 2, 9
    assert B * M > 256 * 1024 and (B * M) % 1024 != 0
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=17, time_sorted=True)
    g = torch.Generator().manual_seed(10)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g)
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    out = _run(L, coeff, table, 0.41, {'events': ev.to(dev), 'num_pos_events': num_pos})
    _against_definition(cfg, ev, num_pos, coeff, table, 0.41, out, 'second trip, tiny image')


def test_no_events_the_table_gradient_is_the_smoothness_terms():
    from motionpriorcmax_amd import LossFactory
    dev = _dev()
    shape, B, nb, k, S = (16, 24), 2, 3, 3, 37
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev = torch.zeros(B, 0, 6)
    g = torch.Generator().manual_seed(11)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    out = _run(L, coeff, table, 0.41, {'events': ev.to(dev), 'num_pos_events': 0})
    # (an empty image has no contrast: the loss is not finite in either implementation, the gradients are the smoothness term's)
    _against_definition(cfg, ev, 0, coeff, table, 0.41, out, 'M = 0', loss_finite=False)


@pytest.mark.parametrize('past', [0, 1])
def test_table_at_the_library_limit_and_one_past_it(past):
    """(S + 1) * k exactly at mpc_pe_table_limit(): the fused node; one past it: the plain-torch route -- both match the definition."""
    from motionpriorcmax_amd import LossFactory, ops, _lib as C
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k = (16, 24), 2, 300, 3, 1
    lim = int(C.lib().mpc_pe_table_limit())
    S = lim - 1 + past
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=18)
    g = torch.Generator().manual_seed(12)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 2.0
    table = torch.cumsum(torch.randn(S + 1, k, generator=g) * 0.02, 0)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    assert ops.pe_table_supported(L._cfg, bg['events'], num_pos, k, S) == (past == 0)
    with ops.KernelTimer() as kt:
        out = _run(L, coeff, table, 0.41, bg)
    names = ' '.join(kt.summary())
    assert ('k_pe_table_grad' in names) == (past == 0), names
    _against_definition(cfg, ev, num_pos, coeff, table, 0.41, out, f'(S + 1) k = limit + {past}')


def test_nine_orders_take_the_plain_torch_route():
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (16, 24), 2, 300, 3, 9, 37
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=19)
    g = torch.Generator().manual_seed(13)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g)
    table = torch.randn(S + 1, k, generator=g) * 0.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    assert not ops.pe_table_supported(L._cfg, bg['events'], num_pos, k, S)
    out = _run(L, coeff, table, 0.41, bg)
    _against_definition(cfg, ev, num_pos, coeff, table, 0.41, out, 'k = 9')


def test_fused_table_step_does_not_synchronise_with_the_host():
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, S = (96, 128), 2, 12000, 5, 3, 1024
    cfg = _cfg(shape, nb)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=20, pad_frac=0.1)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    g = torch.Generator().manual_seed(14)
    cg = (torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0).to(dev).requires_grad_(True)
    tb = (torch.randn(S + 1, k, generator=g) * 0.5).to(dev).requires_grad_(True)
    t_ref = torch.full((1,), 0.41, device=dev)

    def step():
        loss, _, _ = L.calc_per_event_basis(cg, t_ref, ob, k, 'table', basis_table=tb)
        loss.backward()
    step()                                       # warm-up: the one-time set-up of the kernels, the cached bin mid-times
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(tb.grad).all() and float(tb.grad.abs().max()) > 0


def test_table_entry_points_refuse_without_a_launch():
    from motionpriorcmax_amd import LossFactory, ops, _lib as C
    dev = _dev()
    lib = C.lib()
    L = LossFactory.get_loss_calculator('FOCUS', _cfg((16, 24), 3))
    ok = ops.make_shape(L._cfg, 2, 8, 4, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
    warp = ops.make_shape(L._cfg, 2, 8, 4, 0, K=0, extra_flags=C.F_NO_BWD_RECORDS)             # without MPC_F_NO_WARP
    import ctypes
    so, sw = ctypes.byref(ok), ctypes.byref(warp)
    a = torch.zeros(8192, device=dev)
    lim = int(lib.mpc_pe_table_limit())
    P = _p(a)
    with ops.KernelTimer() as kt:
        for S, k, code in ((4, 0, C.E_SHAPE), (4, 9, C.E_SHAPE), (0, 2, C.E_SHAPE), (lim, 1, C.E_UNSUPPORTED)):
            assert lib.mpc_pe_table_warp(so, P, P, P, S, k, P, P, None) == code, (S, k)
            assert lib.mpc_pe_table_grad(so, P, P, S, k, P, P, P, None, P, P, None) == code, (S, k)
            assert lib.mpc_pe_table_grad_ordered(so, P, P, P, S, k, P, P, P, None, P, 1, P, None) == code, (S, k)
            assert lib.mpc_pe_table_basis_grad(so, P, P, P, S, k, P, P, None, P, P, None) == code, (S, k)
            assert lib.mpc_pe_table_supported(so, k, S) == 0
        assert lib.mpc_pe_table_supported(so, 2, 4) == 1 and lib.mpc_pe_table_supported(sw, 2, 4) == 0
        assert lib.mpc_pe_table_supported(None, 2, 4) == 0
        assert lib.mpc_pe_table_warp(sw, P, P, P, 4, 2, P, P, None) == C.E_UNSUPPORTED
        assert lib.mpc_pe_table_grad(sw, P, P, 4, 2, P, P, P, None, P, P, None) == C.E_UNSUPPORTED
        assert lib.mpc_pe_table_grad_ordered(sw, P, P, P, 4, 2, P, P, P, None, P, 1, P, None) == C.E_UNSUPPORTED
        assert lib.mpc_pe_table_basis_grad(sw, P, P, P, 4, 2, P, P, None, P, P, None) == C.E_UNSUPPORTED
        # null pointers, one at a time (grad_out and grad_pos may be null)
        for i in (0, 1, 2, 3, 6, 7):
            args = [so, P, P, P, 4, 2, P, P, None]
            args[i] = None
            assert lib.mpc_pe_table_warp(*args) == C.E_NULL, i
        for i in (0, 1, 2, 5, 6, 7, 9):
            args = [so, P, P, 4, 2, P, P, P, None, P, P, None]
            args[i] = None
            assert lib.mpc_pe_table_grad(*args) == C.E_NULL, i
        for i in (0, 1, 2, 3, 6, 7, 8, 10):
            args = [so, P, P, P, 4, 2, P, P, P, None, P, 1, P, None]
            args[i] = None
            assert lib.mpc_pe_table_grad_ordered(*args) == C.E_NULL, i
        assert lib.mpc_pe_table_grad_ordered(so, P, P, P, 4, 2, P, P, P, None, P, 17, P, None) in (C.E_SHAPE, C.E_UNSUPPORTED)       # split
        for i in (0, 1, 2, 3, 6, 7, 9, 10):
            args = [so, P, P, P, 4, 2, P, P, None, P, P, None]
            args[i] = None
            assert lib.mpc_pe_table_basis_grad(*args) == C.E_NULL, i
        for i in (0, 1, 3, 4):
            args = [P, P, None, P, P, 1, 4, 2, 2, None]
            args[i] = None
            assert lib.mpc_pe_field_basis_grad(*args) == C.E_NULL, i
        assert lib.mpc_pe_field_basis_grad(P, P, None, P, P, 1, 4, 9, 2, None) == C.E_UNSUPPORTED          # k = 9
        assert lib.mpc_pe_field_basis_grad(P, P, None, P, P, 1, 4, 2, 65, None) == C.E_UNSUPPORTED         # nb = 65
        assert lib.mpc_pe_field_basis_grad(P, P, None, P, P, 1, 4, 0, 2, None) == C.E_SHAPE
    assert kt.summary() == {}
    assert float(a.abs().max()) == 0.0


@pytest.mark.parametrize('G,k,nb', [(1, 1, 1), (255, 8, 64), (16400, 3, 5)])
def test_field_basis_gradient_against_einsum(G, k, nb):
    """mpc_pe_field_basis_grad alone against a float64 einsum: one workgroup, a ragged one, and more blocks of cells than the 64
    parts (a second trip of a part's loop); bitwise equal from run to run."""
    from motionpriorcmax_amd import _lib as C
    dev = _dev()
    B = 2
    g = torch.Generator().manual_seed(G)
    gf = torch.randn(B * nb, G, 2, generator=g)
    rows = torch.randn(B * G, 2 * k, generator=g)
    go = torch.tensor([0.7])
    want = 0.7 * torch.einsum('btcd,bcdj->tj', gf.double().view(B, nb, G, 2), rows.double().view(B, G, 2, k))
    outs = []
    gf_d, rows_d, go_d = gf.to(dev), rows.to(dev), go.to(dev)
    for _ in range(2):
        part = torch.empty(nb * 64 * k, dtype=torch.float64, device=dev)
        out = torch.full((nb, k), float('nan'), device=dev)
        C.check(C.lib().mpc_pe_field_basis_grad(_p(gf_d), _p(rows_d), _p(go_d), _p(part), _p(out), B, G, k, nb, None), 'mpc_pe_field_basis_grad')
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    # fp64 sums of exact fp32 products, one rounding to fp32 at the end (and the fp32 grad_out): 2^-23 of the sum of magnitudes
    mag = 0.7 * torch.einsum('btcd,bcdj->tj', gf.double().abs().view(B, nb, G, 2), rows.double().abs().view(B, G, 2, k))
    assert ((outs[0].double() - want).abs() <= 2.0 ** -23 * mag + 1e-30).all()
