"""Where the end-to-end gradient tolerances come from, counted.

The 'l1' objective differentiates |Sobel response| with sign(): a response that is zero up to the rounding of the IWE
sums (Q33.30 integer sums here, fp32 scatter_add in the reference) can come out with either sign, and every event that
votes within the 5x5 footprint of such a pixel then gets a different -- equally valid -- gradient.  That is why the
golden end-to-end tests allow 1e-3 (rel. L2).  This test makes the allowance accountable: every LUT cell whose gradient
differs from the oracle's is EXPLAINED by a near-zero response next to one of its events, the cells that are not
explained agree tightly, and the explained ones are few.  A backward bug in a rarely taken branch would show up as an
unexplained cell.  All other discontinuities of the path (floor(pos + 1e-6), the strict border comparisons) act on event
positions, which are bit-identical on both sides when both warp with the same LUT (same fp32 operations in the same order);
end to end, the events within rounding of them explain their own cells as well.  The rules live in tests/grad_accounting.py."""
import pytest
import torch

from grad_accounting import end_to_end_accounting, lut_accounting

pytestmark = pytest.mark.gpu


def _cfg(shape, nb, norm):
    return dict(image_shape=shape, num_tref=1, num_bins=nb, num_knn=8, smooth_weight=0.0, lut_superpixel_size=4,
                focus_loss_norm=norm, dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True,
                polarity_aware_batching=True, interpolation_scheme='mean', smooth_type='on_flow_to_tref')


@pytest.mark.parametrize('shape,B,M,nb,seed', [((96, 128), 2, 20000, 5, 1), ((480, 640), 1, 200000, 15, 2)])
def test_every_gradient_mismatch_is_explained_by_a_near_zero_response(shape, B, M, nb, seed):
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    H, W = shape
    sp = 4
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=seed, pad_frac=0.02)
    g = torch.Generator().manual_seed(seed)
    lut = torch.randn(B, nb, -(-H // sp), -(-W // sp), 1, 2, generator=g) * 2.0
    t_ref = torch.tensor([0.41])
    cfg = _cfg(shape, nb, 'l1')
    orc = O.FocusLossOracle(**cfg)
    lo = lut.clone().requires_grad_(True)
    fo, iwo, rawo = orc.event_path(ev, lo, t_ref, num_pos)
    fo.backward()
    dev = torch.device('cuda:0')
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    lt = lut.to(dev).requires_grad_(True)
    f, blur, raw = ops.EventFocusFn.apply(lt, ev.to(dev), t_ref.to(dev), L._cfg, num_pos)
    f.backward()
    # every LUT cell that differs from the oracle holds an event next to a near-zero response (tests/grad_accounting.py); the
    # allowance is small, and it is used: the test must not pass because everything is "explained"
    res = lut_accounting(cfg, ev, num_pos, lut, lt.grad.cpu(), lo.grad, blurred=O.gaussian_blur3(rawo.detach()),
                         label=f'LUT {shape}')
    assert res['frac_mismatch'] <= res['frac_explained'] and res['frac_mismatch'] < 0.01 and res['frac_explained'] < 0.25
    # with the sign() out of the way ('l2') the whole gradient agrees tightly
    cfg2 = _cfg(shape, nb, 'l2')
    lo2 = lut.clone().requires_grad_(True)
    f2o, _, _ = O.FocusLossOracle(**cfg2).event_path(ev, lo2, t_ref, num_pos)
    f2o.backward()
    lt2 = lut.to(dev).requires_grad_(True)
    f2, _, _ = ops.EventFocusFn.apply(lt2, ev.to(dev), t_ref.to(dev), LossFactory.get_loss_calculator('FOCUS', cfg2)._cfg, num_pos)
    f2.backward()
    g2o, g2g = lo2.grad, lt2.grad.cpu()
    assert ((g2g - g2o).abs() <= 2e-5 * g2o.abs().max() + 1e-4 * g2o.abs()).all()


@pytest.mark.parametrize('shape,B,M,nb,K', [((192, 256), 2, 60000, 5, 8), ((480, 640), 1, 100000, 15, 32)])
def test_end_to_end_gradient_mismatches_are_explained(shape, B, M, nb, K):
    """The same accounting for d loss / d trajectories through the KNN LUT (dsec.yaml switches, smoothness on): a
    trajectory point may differ from the oracle only if an explained LUT cell averages it (through the device's neighbour sets,
    which the brute-force tests pin; events within rounding of a pixel edge or of the border explain their own cell as well).
    Second case: the DSEC sensor with K = 32 and 15 bins (one sample; the oracle's brute-force KNN takes a minute or two)."""
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    sp = 4
    H, W = shape
    cfg = dict(_cfg(shape, nb, 'l1'), smooth_weight=0.003, num_knn=K)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=5, pad_frac=0.02)
    g = torch.Generator().manual_seed(5)
    coeff = torch.randn(B, 1, 2, H, W, generator=g) * 3.0
    times = torch.cat((torch.tensor([0.37]), O.bin_mid_times(nb)))
    traj = O.trajectories_at(coeff, times, O.tile_mask(shape, 4), 1, 'polynomial')
    to = traj.clone().requires_grad_(True)
    lo, _, _ = O.FocusLossOracle(**cfg).calc(to, times, {'events': ev, 'num_pos_events': num_pos})
    lo.backward()
    dev = torch.device('cuda:0')
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    tg = traj.to(dev).requires_grad_(True)
    lg, _, misc = L.calc(tg, times.to(dev), {'events': ev.to(dev), 'num_pos_events': num_pos})
    lg.backward()
    assert abs(lg.item() - lo.item()) <= 1e-5 * abs(lo.item())
    go, gg = to.grad, tg.grad.cpu()                                    # [B, 1 + nb, n, 2]
    with torch.no_grad():
        lut = ops.KnnLutFn.apply(traj.to(dev), L._cfg)[0].cpu()       # the LUT the events were warped with
        idx = ops.knn_indices(L._cfg, traj.to(dev)).cpu().long()       # and its neighbour sets [B, nb, Q, K]
    # a trajectory point may differ only if a LUT cell averaging it holds an explained event (at K = 32 a point is averaged by
    # ~32 cells per bin and the t_ref row by all of them: half the points have such a cell, so the cap goes on the cells)
    res = end_to_end_accounting(cfg, ev, num_pos, traj, gg, go, blurred=misc['iwes'].cpu(), lut=lut, idx=idx, cap_cells=K > 8,
                                label=f'trajectories {shape} K={K}')
    assert res['frac_mismatch'] < 0.01
