"""UNPINNED extension: the per-event continuous-time basis warp (`FocusLoss.calc_per_event_basis`; BASELINE.json's north_star
names it, the reference has no such path: focus.py:182-195 gathers a binned KNN look-up table).  The HIP path (LDS-tiled vote of
pre-warped rows, contrast kernels, mpc_event_pos_grad + torch for the chain to the coefficient grid) against the DEFINITION
written from the reference's building blocks in oracle/focus_oracle.py (`FocusLossOracle.calc_per_event_basis`)."""
import pytest
import torch

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


@pytest.mark.parametrize('over,basis,k', [
    ({}, 'polynomial', 3), ({'polarity_aware_batching': False, 'scale_iwe_by_dt': False}, 'polynomial', 1),
    ({'focus_loss_norm': 'l2', 'smooth_weight': 0.0}, 'dct', 2), ({'mask_image_border': False}, 'polynomial', 5),
    ({'smooth_weight': 0.0}, 'polynomial', 9),        # more orders than the kernels keep in registers: phi from torch, strided reads
])
@pytest.mark.parametrize('fused', [True, False, 'ordered'])
def test_per_event_basis_against_its_definition(over, basis, k, fused):
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb = (96, 128), 2, 12000, 5
    cfg = _cfg(shape, nb, **over)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=11, pad_frac=0.1)
    g = torch.Generator().manual_seed(3)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=g) * 4.0          # some events leave the image
    batch = {'events': ev, 'num_pos_events': num_pos}
    co = coeff.clone().requires_grad_(True)
    lo, _, mo = O.FocusLossOracle(**cfg).calc_per_event_basis(co, 0.41, batch, k, basis)
    lo.backward()
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    cg = coeff.to(dev).requires_grad_(True)
    bg = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if fused == 'ordered':
        bg = L.order_events(bg)                  # rows permuted inside the polarity blocks + offsets: same loss, LDS backward
    lg, log, mg = L.calc_per_event_basis(cg, 0.41, bg, k, basis, fused=bool(fused))
    lg.backward()
    assert abs(lg.item() - lo.item()) <= 1e-5 * abs(lo.item()), (lg.item(), lo.item())
    iw = mo['iwes'].reshape(mg['iwes'].shape)
    assert (mg['iwes'].cpu() - iw).abs().max() <= 1e-5 * iw.abs().max()
    # gradient: relative L2 (an event next to a pixel whose Sobel response is zero up to rounding may take the other sign())
    go, gg = co.grad, cg.grad.cpu()
    assert torch.isfinite(gg).all() and go.abs().max() > 0
    sign_free = cfg['focus_loss_norm'] == 'l2'
    assert (gg - go).norm() / go.norm() < (1e-4 if sign_free else 2e-3), float((gg - go).norm() / go.norm())
    from grad_accounting import per_event_accounting
    per_event_accounting(cfg, ev, num_pos, coeff, 0.41, k, basis, gg, go, label=f'per-event {over} {basis} k={k} fused={fused}')
    # only the tile centres receive gradient (trajectories.py:3-13: the coefficients are sampled there)
    from motionpriorcmax_amd.utils import get_optical_flow_tile_mask
    assert float(gg[..., ~get_optical_flow_tile_mask(shape, 4)].abs().max()) == 0.0


def test_per_event_basis_is_reproducible_and_zero_coefficients_are_the_identity_warp():
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k = (96, 128), 2, 9000, 5, 3
    cfg = _cfg(shape, nb, smooth_weight=0.0)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=5)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    z = torch.zeros(B, 1, 2 * k, *shape, device=dev)
    l0, _, m0 = L.calc_per_event_basis(z, 0.3, batch, k)
    lut = torch.zeros(B, nb, shape[0] // 4, shape[1] // 4, 1, 2, device=dev)
    f, iw, _ = ops.EventFocusFn.apply(lut, batch['events'], torch.tensor([0.3], device=dev), L._cfg, num_pos)
    assert torch.equal(l0, f) and torch.equal(m0['iwes'].reshape(iw.shape), iw)
    g = torch.Generator().manual_seed(1)
    c = (torch.randn(B, 1, 2 * k, *shape, generator=g) * 3).to(dev)
    outs = []
    for _ in range(2):
        cg = c.clone().requires_grad_(True)
        l, _, _ = L.calc_per_event_basis(cg, 0.3, batch, k)
        l.backward()
        outs.append((l.detach().clone(), cg.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0])          # forward: integer accumulation, bitwise reproducible
    assert torch.isfinite(outs[0][1]).all()
    # with the bucket-ordered layout the backward is bitwise reproducible too (LDS fixed point, no global atomics)
    ob = L.order_events(batch)
    outs = []
    for _ in range(2):
        cg = c.clone().requires_grad_(True)
        l, _, _ = L.calc_per_event_basis(cg, 0.3, ob, k)
        l.backward()
        outs.append((l.detach().clone(), cg.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # ... and the forward does not care about the row order inside a polarity block: same loss, bit for bit
    cg = c.clone().requires_grad_(True)
    lp, _, _ = L.calc_per_event_basis(cg, 0.3, batch, k)
    assert torch.equal(lp.detach(), outs[0][0])
    for kk, basis in ((9, 'polynomial'), (8, 'dct')):
        c9 = (torch.randn(B, 1, 2 * kk, *shape, generator=g) * 0.5).to(dev)
        la, _, _ = L.calc_per_event_basis(c9, 0.3, batch, kk, basis)
        lb, _, _ = L.calc_per_event_basis(c9, 0.3, ob, kk, basis)
        assert torch.equal(la, lb), (kk, basis, float(la), float(lb))


# ---- directed tests of the branches one geometry never reaches (the randomised ones: tools/fuzz_per_event.py) ----------------
def _oracle64(cfg, ev, num_pos, coeff, t_ref, k, basis, gscale=1.0):
    from oracle import focus_oracle as O
    co = coeff.double().requires_grad_(True)
    lo, _, _ = O.FocusLossOracle(**cfg).calc_per_event_basis(co, float(t_ref), {'events': ev.double(), 'num_pos_events': num_pos}, k, basis)
    (lo * gscale).backward()
    return float(lo.detach()), co.grad


def _against_oracle(cfg, ev, num_pos, coeff, t_ref, k, basis, lg, mg, gg, label, gscale=1.0):
    """The rules of test_per_event_basis_against_its_definition.  For a sign-free objective the relative L2 bound is 1e-4; where
    the fp32 oracle itself misses that against float64, the case is judged against float64 at 4 times the fp32 oracle's own
    distance (the rule of tests/test_cvx_traj_host.py), both figures printed."""
    from oracle import focus_oracle as O
    from grad_accounting import per_event_accounting
    from motionpriorcmax_amd.utils import get_optical_flow_tile_mask
    co = coeff.clone().requires_grad_(True)
    lo, _, mo = O.FocusLossOracle(**cfg).calc_per_event_basis(co, t_ref, {'events': ev, 'num_pos_events': num_pos}, k, basis)
    (lo * gscale).backward()
    assert abs(lg.item() - lo.item()) <= 1e-5 * abs(lo.item()), (label, lg.item(), lo.item())
    iw = mo['iwes'].reshape(mg['iwes'].shape)
    assert (mg['iwes'].cpu() - iw).abs().max() <= 1e-5 * iw.abs().max(), label
    go, gg = co.grad, gg.cpu()
    assert torch.isfinite(gg).all() and go.abs().max() > 0
    res = per_event_accounting(cfg, ev, num_pos, coeff, t_ref, k, basis, gg, go, label=label)
    if cfg['focus_loss_norm'] == 'l2' or cfg.get('loss_type') == 'variance':
        r32 = float((gg - go).norm() / go.norm())
        print(f'{label}: relative L2 of the gradient {r32:.3e} (bound 1e-4)')
        if not r32 < 1e-4:
            _, g64 = _oracle64(cfg, ev, num_pos, coeff, np_f32(t_ref), k, basis, gscale)
            d_or, d_dev = float((go.double() - g64).norm() / g64.norm()), float((gg.double() - g64).norm() / g64.norm())
            print(f'{label}: against float64: fp32 oracle {d_or:.3e}, device {d_dev:.3e}')
            assert d_or >= 1e-4 and d_dev <= 4 * d_or, (label, r32, d_or, d_dev)
    s = cfg['lut_superpixel_size']
    assert float(gg[..., ~get_optical_flow_tile_mask(cfg['image_shape'], s)].abs().max()) == 0.0
    return res


def _pe_shape(L, B, M, num_pos):
    from motionpriorcmax_amd import ops, _lib as C
    Mp = num_pos if L._cfg.polarity_split else M
    return ops.make_shape(L._cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)


def _run(L, coeff, t_ref, batch, k, basis='polynomial', timer=False):
    from motionpriorcmax_amd import ops
    cg = coeff.to(batch['events'].device).requires_grad_(True)
    if timer:
        with ops.KernelTimer() as kt:
            lg, _, mg = L.calc_per_event_basis(cg, t_ref, batch, k, basis)
            lg.backward()
        return lg.detach(), mg, cg.grad, kt.summary()
    lg, _, mg = L.calc_per_event_basis(cg, t_ref, batch, k, basis)
    lg.backward()
    return lg.detach(), mg, cg.grad, None


@pytest.mark.parametrize('k', [3, 4])
def test_ordered_backward_at_the_lds_limit(k):
    """96 x 128 at sp = 2: 48 x 64 cells.  api.hip: cstrip_rows = 48 KB / (wq * 16) = 48 = hq, one strip; k_pe_accum needs
    cstrip_rows * wq * 2k * 8 bytes of LDS against 150 KB: k = 3 -> 147456 (the largest launch that fits), k = 4 -> 196608 (the
    ordered batch takes the atomic backward)."""
    import ctypes
    import os
    from motionpriorcmax_amd import LossFactory, _lib as C
    from oracle import focus_oracle as O
    if os.environ.get('MPC_EV_CSTRIP_KB'):
        pytest.skip('MPC_EV_CSTRIP_KB is set: the strip rule this test derives its expectation from is overridden')
    dev = _dev()
    shape, B, M, nb, sp = (96, 128), 1, 8000, 5, 2
    hq, wq = shape[0] // sp, shape[1] // sp
    rows = min((48 * 1024) // (wq * 16), hq)
    rows = -(-hq // -(-hq // rows))
    lds = rows * wq * 2 * k * 8
    assert lds == {3: 147456, 4: 196608}[k]
    want = 1 if lds <= 150 * 1024 else 0
    cfg = _cfg(shape, nb, lut_superpixel_size=sp, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=21, pad_frac=0.1)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(4)) * 3.0
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    sh = _pe_shape(L, B, M, num_pos)
    assert int(C.lib().mpc_pe_grad_ordered_supported(ctypes.byref(sh), k)) == want
    lg, mg, gg, ran = _run(L, coeff, 0.41, ob, k, timer=True)
    assert ('k_pe_accum' in ran, 'k_pe_grad' in ran) == ((True, False) if want else (False, True)), sorted(ran)
    _against_oracle(cfg, ev, num_pos, coeff, 0.41, k, 'polynomial', lg, mg, gg, f'LDS limit k={k}')
    l2, _, g2, _ = _run(L, coeff, 0.41, ob, k)
    assert torch.equal(l2, lg)
    if want:
        assert torch.equal(g2, gg)          # LDS fixed point: bitwise reproducible


def test_ordered_backward_with_more_parts_than_ranges():
    """nb = 1: a strip has 2 row ranges (one per polarity) and split = 16 workgroups -- 14 of them have nothing but zeros to write."""
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k = (96, 128), 2, 6000, 1, 2
    cfg = _cfg(shape, nb, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=22, pad_frac=0.1)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(5)) * 3.0
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    strips = ops._lut_strips(_pe_shape(L, B, M, num_pos), dev)
    assert max(1, min(16, 512 // (B * strips))) == 16 and 2 * nb < 16, strips
    lg, mg, gg, ran = _run(L, coeff, 0.41, ob, k, timer=True)
    assert 'k_pe_accum' in ran and 'k_pe_grad' not in ran
    _against_oracle(cfg, ev, num_pos, coeff, 0.41, k, 'polynomial', lg, mg, gg, 'split 16, 2 ranges')


def test_ordered_backward_with_one_part_per_strip():
    """split = min(16, 512 // (B * strips)) = 1 needs B * strips > 256.  At 480 x 640 (the DSEC image) with sp = 2 a strip has
    48 KB / (320 * 16) = 9 rows of cells -> 27 strips: the smallest batch with split = 1 is B = 256 // strips + 1 = 10.
    (strips ~ cells / 3072 while a row of cells fits a strip, so B = 3 needs 86 strips: 264 k cells -- 860 x 1032 at sp = 2, more
    pixels than these ten images -- or an image more than 3072 pixels wide, 172 x 3074, a shape nothing else in the suite runs the
    vote and contrast kernels at.  Ten DSEC-size images with 1500 events each cost the oracle 0.3 s.)"""
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    dev = _dev()
    shape, M, nb, k, sp = (480, 640), 1500, 2, 1, 2
    cfg = _cfg(shape, nb, lut_superpixel_size=sp, focus_loss_norm='l2', smooth_weight=0.0)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    strips = ops._lut_strips(_pe_shape(L, 1, M, M // 2), dev)
    B = 256 // strips + 1
    assert strips == ops._lut_strips(_pe_shape(L, B, M, M // 2), dev)
    assert max(1, min(16, 512 // (B * strips))) == 1 and max(1, min(16, 512 // ((B - 1) * strips))) == 2, (B, strips)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=23)
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(6)) * 3.0
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    lg, mg, gg, ran = _run(L, coeff, 0.41, ob, k, timer=True)
    assert 'k_pe_accum' in ran and 'k_pe_grad' not in ran
    _against_oracle(cfg, ev, num_pos, coeff, 0.41, k, 'polynomial', lg, mg, gg, f'split 1 (B={B}, {strips} strips)')


@pytest.mark.parametrize('shape,sp,k,nb,fused,basis', [
    ((10, 14), 4, 2, 3, False, 'polynomial'),         # the torch cross-check: TileCoeffRowsFn + GatherRowsFn
    ((10, 14), 4, 2, 65, True, 'polynomial'),         # more than 64 bins: TileCoeffRowsFn + PerEventBasisFocusFn + torch smoothness
    ((9, 13), 3, 9, 3, 'ordered', 'dct'),             # more than 8 orders, ordered batch: TileCoeffRowsFn + the LDS backward
    ((10, 14), 4, 2, 3, True, 'polynomial'),          # the fused node at the same shape: k_tile_rows writes the zeros itself
])
def test_per_event_basis_where_a_tile_has_no_centre(shape, sp, k, nb, fused, basis):
    """Regression: 0 < H % sp <= sp // 2 (10 % 4 = 2, 14 % 4 = 2; 13 % 3 = 1) leaves the last row / column of cells without a
    centre in the image.  TileCoeffRowsFn -- the route of fused=False, k > 8 and num_bins > 64 -- sliced the centres out of the grid
    and raised on the reshape to [B * hq * wq, 2k] at every such shape (tools/fuzz_per_event.py `30 24`: cases 2, 5, 10, 20, 26 among
    others).  Here: B = 2, S = 2 scales, M = 600 (seed 41, 10 % padding), coefficients seed 7 times 1.5, t_ref = 0.41, 'l2' norm,
    smooth_weight 0.003, loss * -2.5; one event is put into the cell without a centre.  Against the oracle, with exact zeros where
    the gradient of such a cell would have gone."""
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    B, S, M = 2, 2, 600
    cfg = _cfg(shape, nb, lut_superpixel_size=sp, focus_loss_norm='l2')
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=41, pad_frac=0.1)
    ev[0, 0, :2] = torch.tensor([shape[0] - 0.5, shape[1] - 0.5])
    coeff = torch.randn(B, S, 2 * k, *shape, generator=torch.Generator().manual_seed(7)) * 1.5
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if fused == 'ordered':
        batch = L.order_events(batch)
    cg = coeff.to(dev).requires_grad_(True)
    lg, _, mg = L.calc_per_event_basis(cg, 0.41, batch, k, basis, fused=bool(fused))
    (lg * -2.5).backward()
    _against_oracle(cfg, ev, num_pos, coeff, 0.41, k, basis, lg.detach(), mg, cg.grad, f'no centre {shape} sp={sp} k={k} nb={nb} fused={fused}',
                    gscale=-2.5)
    hq, wq = -(-shape[0] // sp), -(-shape[1] // sp)
    gg = cg.grad.cpu()
    if len(range(sp // 2, shape[0], sp)) < hq:
        assert float(gg[..., (hq - 1) * sp:, :].abs().max()) == 0.0
    if len(range(sp // 2, shape[1], sp)) < wq:
        assert float(gg[..., (wq - 1) * sp:].abs().max()) == 0.0


def _p(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('B,S,c2,H,W,tile', [(2, 3, 6, 10, 14, 4), (1, 2, 2, 9, 13, 3), (1, 1, 16, 5, 7, 8), (2, 1, 4, 8, 12, 1)])
def test_tile_rows_and_their_adjoint_against_numpy(B, S, c2, H, W, tile):
    """mpc_pe_tile_rows / mpc_pe_tile_rows_bwd through the C ABI: tiles without a centre (10 x 14 at 4, 9 x 13 at 3), a tile larger
    than the image (its centre (4, 4) lies inside 5 x 7), tile = 1, W % 4 != 0 and == 0."""
    import numpy as np
    from motionpriorcmax_amd import _lib as C
    dev = _dev()
    hq, wq = -(-H // tile), -(-W // tile)
    rng = np.random.default_rng(B * 1000 + tile)
    grid = rng.standard_normal((B, S, c2, H, W)).astype(np.float32)
    gd = torch.from_numpy(grid).to(dev)
    rows = torch.full((B * hq * wq, c2), float('nan'), device=dev)
    C.check(C.lib().mpc_pe_tile_rows(_p(gd), _p(rows), B, S, c2, H, W, tile, None), 'mpc_pe_tile_rows')
    want = np.zeros((B, hq, wq, c2))
    part = np.zeros((B, hq, wq, c2))                    # the largest partial sum, for the bound
    ys, xs = np.arange(tile // 2, H, tile), np.arange(tile // 2, W, tile)
    for s in range(S):                                  # the kernel's order of addition: scales ascending, fp32
        acc = (want[:, :len(ys), :len(xs)] + grid[:, s][:, :, ys][:, :, :, xs].transpose(0, 2, 3, 1).astype(np.float64))
        want[:, :len(ys), :len(xs)] = acc
        part = np.maximum(part, np.abs(want))
    got = rows.cpu().numpy().reshape(B, hq, wq, c2).astype(np.float64)
    assert np.isfinite(got).all()
    ulp = np.spacing(part.astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= 2 * ulp).all(), float(np.abs(got - want).max())
    assert (got[:, len(ys):] == 0).all() and (got[:, :, len(xs):] == 0).all()        # no centre: exact zeros
    # adjoint: a bitwise copy to every scale, zeros elsewhere, every element written
    grows = torch.from_numpy(rng.standard_normal((B * hq * wq, c2)).astype(np.float32)).to(dev)
    gg = torch.full((B, S, c2, H, W), float('nan'), device=dev)
    C.check(C.lib().mpc_pe_tile_rows_bwd(_p(grows), _p(gg), B, S, c2, H, W, tile, None), 'mpc_pe_tile_rows_bwd')
    wantb = torch.zeros(B, S, c2, H, W, device=dev)
    src = grows.view(B, hq, wq, c2)[:, :len(ys), :len(xs)].permute(0, 3, 1, 2)
    wantb[:, :, :, tile // 2::tile, tile // 2::tile] = src[:, None]
    assert torch.equal(gg, wantb)


@pytest.mark.parametrize('G', [1, 255, 257])
@pytest.mark.parametrize('k,nb', [(1, 1), (8, 64), (1, 64), (8, 1)])
def test_basis_field_and_rows_grad_finish_against_einsum(G, k, nb):
    import numpy as np
    from motionpriorcmax_amd import _lib as C
    dev = _dev()
    B = 2
    rng = np.random.default_rng(G * 100 + k * 10 + nb)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)          # noqa: E731
    rows, phim = f32(B, G, 2, k), f32(nb, k)
    rd, pd = torch.from_numpy(rows).to(dev), torch.from_numpy(phim).to(dev)
    field = torch.full((B * nb, G, 2), float('nan'), device=dev)
    C.check(C.lib().mpc_pe_basis_field(_p(rd), _p(pd), _p(field), B, G, k, nb, None), 'mpc_pe_basis_field')
    want = np.einsum('bgdj,tj->btgd', rows.astype(np.float64), phim.astype(np.float64))
    big = np.abs(rows).max() * np.abs(phim).max()
    err = np.abs(field.cpu().numpy().reshape(B, nb, G, 2) - want).max()
    assert err <= k * nb * 2.0 ** -23 * big, (err, big)
    gfield, go = f32(B, nb, G, 2), np.float32(-2.5)
    gfd, god = torch.from_numpy(gfield).to(dev), torch.tensor([float(go)], device=dev)
    for split in (0, 1, 16):
        parts = f32(max(split, 1), B, G, 2, k)
        ptd = torch.from_numpy(parts).to(dev)
        for with_field in (True, False):
            for with_go in (True, False):
                out = torch.full((B * G, 2 * k), float('nan'), device=dev)
                C.check(C.lib().mpc_pe_rows_grad_finish(_p(ptd) if split else None, split, _p(gfd) if with_field else None,
                                                        _p(pd) if with_field else None, _p(god) if with_go else None, _p(out), B, G, k, nb, None),
                        'mpc_pe_rows_grad_finish')
                w = parts[:split].astype(np.float64).sum(0) if split else np.zeros((B, G, 2, k))
                bigw = np.abs(parts).max() if split else 0.0
                if with_field:
                    w = w + (float(go) if with_go else 1.0) * np.einsum('btgd,tj->bgdj', gfield.astype(np.float64), phim.astype(np.float64))
                    bigw = max(bigw, np.abs(gfield).max() * np.abs(phim).max() * (abs(float(go)) if with_go else 1.0))
                e = np.abs(out.cpu().numpy().reshape(B, G, 2, k) - w).max()
                # (k * nb * 2^-23 of the largest product, as for the field; the `split` partial results are `split` more terms of the sum)
                assert e <= (k * nb + split) * 2.0 ** -23 * bigw, (split, with_field, with_go, e, bigw)


def test_tile_operators_refuse_without_a_launch():
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    L = C.lib()
    a = torch.zeros(4096, device=dev)
    with ops.KernelTimer() as kt:
        assert L.mpc_pe_basis_field(_p(a), _p(a), _p(a), 1, 4, 9, 2, None) == C.E_UNSUPPORTED          # k = 9
        assert L.mpc_pe_basis_field(_p(a), _p(a), _p(a), 1, 4, 2, 65, None) == C.E_UNSUPPORTED         # nb = 65
        assert L.mpc_pe_rows_grad_finish(_p(a), 1, _p(a), _p(a), None, _p(a), 1, 4, 9, 2, None) == C.E_UNSUPPORTED
        assert L.mpc_pe_rows_grad_finish(_p(a), 1, _p(a), _p(a), None, _p(a), 1, 4, 2, 65, None) == C.E_UNSUPPORTED
        assert L.mpc_pe_basis_field(None, _p(a), _p(a), 1, 4, 2, 2, None) == C.E_NULL
        assert L.mpc_pe_basis_field(_p(a), None, _p(a), 1, 4, 2, 2, None) == C.E_NULL
        assert L.mpc_pe_basis_field(_p(a), _p(a), None, 1, 4, 2, 2, None) == C.E_NULL
        assert L.mpc_pe_rows_grad_finish(_p(a), 1, None, None, None, None, 1, 4, 2, 2, None) == C.E_NULL       # no output
        assert L.mpc_pe_rows_grad_finish(None, 1, None, None, None, _p(a), 1, 4, 2, 2, None) == C.E_NULL       # parts missing, split = 1
        assert L.mpc_pe_rows_grad_finish(_p(a), 1, _p(a), None, None, _p(a), 1, 4, 2, 2, None) == C.E_NULL     # a field gradient without phim
        assert L.mpc_pe_tile_rows(None, _p(a), 1, 1, 2, 8, 8, 4, None) == C.E_NULL
        assert L.mpc_pe_tile_rows(_p(a), None, 1, 1, 2, 8, 8, 4, None) == C.E_NULL
        assert L.mpc_pe_tile_rows_bwd(None, _p(a), 1, 1, 2, 8, 8, 4, None) == C.E_NULL
        assert L.mpc_pe_tile_rows_bwd(_p(a), None, 1, 1, 2, 8, 8, 4, None) == C.E_NULL
        assert L.mpc_pe_tile_rows(_p(a), _p(a), 1, 1, 3, 8, 8, 4, None) == C.E_SHAPE                    # odd c2
        assert L.mpc_pe_tile_rows_bwd(_p(a), _p(a), 1, 1, 3, 8, 8, 4, None) == C.E_SHAPE
    assert kt.summary() == {}
    assert float(a.abs().max()) == 0.0


def test_tile_rows_adjoint_second_trip_of_the_grid_stride_loop():
    """The launch is capped at 65536 workgroups of 256 threads, one thread per group of four pixels: B * S * c2 * H * ceil(W / 4) =
    2 * 2 * 16 * 512 * 513 = 16809984 groups > 65536 * 256 = 16777216, so the last 32768 groups are the loop's second trip; W = 2049
    takes the scalar stores with a ragged last group.  An exact copy: no tolerance."""
    from motionpriorcmax_amd import _lib as C
    dev = _dev()
    B, S, c2, H, W, tile = 2, 2, 16, 512, 2049, 4
    hq, wq = -(-H // tile), -(-W // tile)
    assert B * S * c2 * H * ((W + 3) // 4) > 65536 * 256 >= B * S * c2 * (H - 1) * ((W + 3) // 4) and W % 4 != 0
    grows = torch.randn(B * hq * wq, c2, generator=torch.Generator().manual_seed(9)).to(dev)
    gg = torch.full((B, S, c2, H, W), float('nan'), device=dev)
    C.check(C.lib().mpc_pe_tile_rows_bwd(_p(grows), _p(gg), B, S, c2, H, W, tile, None), 'mpc_pe_tile_rows_bwd')
    want = torch.zeros(B, S, c2, H, W, device=dev)
    nx = len(range(tile // 2, W, tile))                 # 512 of the 513 columns of cells have a centre (2049 % 4 = 1)
    want[:, :, :, tile // 2::tile, tile // 2::tile] = grows.view(B, hq, wq, c2)[:, :, :nx].permute(0, 3, 1, 2)[:, None]
    assert torch.equal(gg, want)


def test_ordered_backward_with_small_event_weights():
    """Weights of 1e-4 (column 5) make every phi * gradient product that k_pe_accum converts to Q33.30 small: one rounding of
    2^-31 per row added, times |GCOEF * grad_out| once the sum is scaled.  Per tile coefficient the allowed difference from the
    float64 definition is the accounting's fp32 rule (POINT_TIGHT) plus n_rows_in_cell * 2^-31 * |GCOEF * grad_out| * max |phi|.
    The bound is derived, not tuned: k_pe_accum converts with pe_to_fixed, which rounds to nearest (a conversion that truncates
    towards zero loses up to 2^-30 per row, always the same way, and misses it).  The worst ratio is printed: 0.705 on an MI355X
    (1.276 truncating; tests/test_pe_fixed_rounding_host.py reproduces both figures on the host)."""
    from grad_accounting import POINT_TIGHT
    from motionpriorcmax_amd import LossFactory
    from oracle import focus_oracle as O
    dev = _dev()
    shape, B, M, nb, k, sp, t_ref = (96, 128), 2, 12000, 5, 3, 4, 0.41
    cfg = _cfg(shape, nb, focus_loss_norm='l2', smooth_weight=0.0)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=31, pad_frac=0.1)
    ev[..., 5] *= 1e-4
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(8)) * 2.0
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ob = L.order_events({'events': ev.to(dev), 'num_pos_events': num_pos})
    lg, mg, gg, ran = _run(L, coeff, t_ref, ob, k, timer=True)
    assert 'k_pe_accum' in ran and 'k_pe_grad' not in ran
    l64, g64 = _oracle64(cfg, ev, num_pos, coeff, np_f32(t_ref), k, 'polynomial')
    # (the forward votes in Q33.30 too: taps of 1e-4 and less are truncated there, and the loss -- not this test's subject -- moves
    # by parts in 1e5; printed, the gradient below is what is asserted)
    print(f'small weights: loss {lg.item()!r} against float64 {l64!r}: relative {abs(lg.item() - l64) / abs(l64):.2e}')
    hq, wq = shape[0] // sp, shape[1] // sp
    m = O.tile_mask(shape, sp)
    sel = lambda g: g[:, 0][..., m].reshape(B, 2 * k, hq, wq).double()          # noqa: E731
    got, want = sel(gg.cpu()), sel(g64)
    valid = ev[..., 5] != 0
    iy, ix = (ev[..., 0] / sp).floor().long().clamp(0, hq - 1), (ev[..., 1] / sp).floor().long().clamp(0, wq - 1)
    n_rows = torch.zeros(B, hq * wq).scatter_add_(1, iy * wq + ix, valid.float()).reshape(B, 1, hq, wq).double()
    val = 1.0 / l64                                     # 'l2' objective: GCOEF = -1 / val^2 / N (contrast.hip)
    gcoef = 1.0 / (val * val) / (B * 2 * shape[0] * shape[1])
    phi_max = float((O.basis_matrix(torch.tensor([np_f32(t_ref)]), k, 'polynomial')
                     - O.basis_matrix(ev[..., 2][valid], k, 'polynomial')).abs().max())
    allowed = POINT_TIGHT[0] * want.abs().max() + POINT_TIGHT[1] * want.abs() + n_rows * 2.0 ** -31 * gcoef * 1.0 * phi_max
    ratio = ((got - want).abs() / allowed).max()
    print(f'small weights: worst |difference| / allowed = {float(ratio):.3f} (fixed-point share of the bound up to '
          f'{float((n_rows * 2.0 ** -31 * gcoef * phi_max / allowed).max()):.3f})')
    assert ratio <= 1.0, float(ratio)


def np_f32(x):
    import numpy as np
    return float(np.float32(x))
