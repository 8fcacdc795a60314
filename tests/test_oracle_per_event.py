"""The DEFINITION of the per-event basis warp (`FocusLossOracle.calc_per_event_basis`) where a tile has no centre: with
0 < H % sp <= sp // 2 the look-up table has ceil(H / sp) rows of cells but the grid only (H - sp // 2 + sp - 1) // sp rows of
tile centres (W likewise).  Cells without a centre carry zero coefficients.  Checked against a literal per-event Python loop
(float64, no tensor indexing: every event, tap and cell spelt out)."""
import math

import pytest
import torch

from oracle import focus_oracle as O


def _loop_definition(coeff, t_ref, ev, num_pos, shape, sp, nb, k, basis, scale_by_dt, mask_border, split):
    """-> (raw IWE [B, P, H, W], smoothness field [B * nb, 2, hq, wq]) as nested Python loops over float64 scalars."""
    H, W = shape
    hq, wq = -(-H // sp), -(-W // sp)
    B, M = ev.shape[:2]
    S = coeff.shape[1]

    def phi(t, j):               # basis.py:18-31, order j = 1..k
        return t ** j if basis == 'polynomial' else math.sqrt(2.0) * math.cos(math.pi / 2.0 * (2 * t + 1) * j)

    def tile_coeff(b, d, iy, ix, j):
        y, x = iy * sp + sp // 2, ix * sp + sp // 2
        if y >= H or x >= W:
            return 0.0           # the tile has no centre inside the image
        return sum(float(coeff[b, s, d * k + j - 1, y, x]) for s in range(S))

    P = 2 if split else 1
    raw = torch.zeros(B, P, H, W, dtype=torch.float64)
    for b in range(B):
        for i in range(M):
            y, x, t, _, _, valid = (float(v) for v in ev[b, i])
            iy, ix = min(max(math.floor(y / sp), 0), hq - 1), min(max(math.floor(x / sp), 0), wq - 1)
            wy = y + sum(tile_coeff(b, 0, iy, ix, j) * (phi(t_ref, j) - phi(t, j)) for j in range(1, k + 1))
            wx = x + sum(tile_coeff(b, 1, iy, ix, j) * (phi(t_ref, j) - phi(t, j)) for j in range(1, k + 1))
            w = valid * ((1 - min(max(abs(t - t_ref), 0.0), 1.0)) if scale_by_dt else 1.0)
            if mask_border and (wy > H or wx > W or wy < 0 or wx < 0):
                w = 0.0
            y0, x0 = math.floor(wy + 1e-6), math.floor(wx + 1e-6)
            fy, fx = wy - y0, wx - x0
            pol = 1 if (split and i >= num_pos) else 0
            for yy, xx, v in ((y0, x0, (1 - fy) * (1 - fx)), (y0 + 1, x0, fy * (1 - fx)), (y0, x0 + 1, (1 - fy) * fx), (y0 + 1, x0 + 1, fy * fx)):
                if 0 <= yy < H and 0 <= xx < W:
                    raw[b, pol, yy, xx] += v * w
    field = torch.zeros(B * nb, 2, hq, wq, dtype=torch.float64)
    tm = [float(v) for v in O.bin_mid_times(nb)]
    for b in range(B):
        for it in range(nb):
            for d in range(2):
                for iy in range(hq):
                    for ix in range(wq):
                        field[b * nb + it, d, iy, ix] = sum(tile_coeff(b, d, iy, ix, j) * (phi(t_ref, j) - phi(tm[it], j)) for j in range(1, k + 1))
    return raw, field


@pytest.mark.parametrize('shape,sp,S,k,basis,split', [
    ((10, 14), 4, 2, 2, 'polynomial', True),      # 10 % 4 = 2 <= 2 and 14 % 4 = 2: no centre in the last row and column (hq, wq = 3, 4; 2 x 3 centres)
    ((9, 13), 3, 1, 3, 'dct', False),             # 9 divides; 13 % 3 = 1 <= 1: no centre in the last column only
])
def test_per_event_definition_where_a_tile_has_no_centre(shape, sp, S, k, basis, split):
    H, W = shape
    B, M, nb, t_ref = 2, 60, 3, 0.25
    hq, wq = -(-H // sp), -(-W // sp)
    hc, wc = len(range(sp // 2, H, sp)), len(range(sp // 2, W, sp))
    assert (hc, wc) != (hq, wq)
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=7, pad_frac=0.1)
    ev[0, 0, :2] = torch.tensor([H - 0.5, W - 0.5])          # one event certainly in the cell without a centre
    g = torch.Generator().manual_seed(2)
    coeff = torch.randn(B, S, 2 * k, H, W, generator=g) * 2.0
    cfg = dict(image_shape=shape, num_tref=1, num_bins=nb, num_knn=1, smooth_weight=0.05, lut_superpixel_size=sp, focus_loss_norm='l2',
               dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=split, interpolation_scheme='mean',
               smooth_type='on_flow_to_tref')
    co = coeff.double().requires_grad_(True)
    loss, log, misc = O.FocusLossOracle(**cfg).calc_per_event_basis(co, t_ref, {'events': ev.double(), 'num_pos_events': num_pos}, k, basis)
    loss.backward()
    raw, field = _loop_definition(coeff.double(), t_ref, ev.double(), num_pos, shape, sp, nb, k, basis, True, True, split)
    blur = O.gaussian_blur3(raw)
    want_iwe = blur if split else blur[:, 0]
    assert torch.allclose(misc['iwes'], want_iwe, rtol=0, atol=1e-12 * float(want_iwe.abs().max()))
    want = 1 / O.contrast_value(want_iwe, 'gradient_magnitude', 'l2') + 0.05 * O.smoothness(field)
    assert abs(float(loss.detach()) - float(want)) <= 1e-12 * abs(float(want)), (float(loss.detach()), float(want))
    # no gradient off the tile centres (the cells without a centre have none to receive it), some gradient on them
    grad = co.grad
    m = O.tile_mask(shape, sp)
    assert float(grad[..., ~m].abs().max()) == 0.0
    assert float(grad[..., m].abs().max()) > 0
    # fp32, as the tests run it: no exception, same value up to fp32 rounding
    l32, _, _ = O.FocusLossOracle(**cfg).calc_per_event_basis(coeff, t_ref, {'events': ev, 'num_pos_events': num_pos}, k, basis)
    assert abs(float(l32) - float(want)) <= 1e-4 * abs(float(want))


def test_per_event_definition_is_unchanged_where_every_tile_has_a_centre():
    """Where every tile has a centre (divisible shapes, and H % sp > sp // 2) the padding branch is not taken; the definition still
    agrees with the loop at fp32 accuracy."""
    for shape, sp in (((8, 12), 4), ((11, 15), 4), ((9, 12), 3)):
        H, W = shape
        assert (len(range(sp // 2, H, sp)), len(range(sp // 2, W, sp))) == (-(-H // sp), -(-W // sp))
        ev, num_pos = O.synth_events(1, 40, shape, 2, seed=1)
        coeff = torch.randn(1, 1, 4, H, W, generator=torch.Generator().manual_seed(0))
        cfg = dict(image_shape=shape, num_tref=1, num_bins=2, num_knn=1, smooth_weight=0.01, lut_superpixel_size=sp, focus_loss_norm='l1',
                   dist_norm='l2', scale_iwe_by_dt=False, mask_image_border=False, polarity_aware_batching=True,
                   interpolation_scheme='mean', smooth_type='on_flow_to_tref')
        loss, _, _ = O.FocusLossOracle(**cfg).calc_per_event_basis(coeff, 0.5, {'events': ev, 'num_pos_events': num_pos}, 2)
        raw, field = _loop_definition(coeff.double(), 0.5, ev.double(), num_pos, shape, sp, 2, 2, 'polynomial', False, False, True)
        want = 1 / O.contrast_value(O.gaussian_blur3(raw), 'gradient_magnitude', 'l1') + 0.01 * O.smoothness(field)
        assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
