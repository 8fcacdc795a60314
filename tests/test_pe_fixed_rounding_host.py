"""Host emulation of the Q33.30 accumulation of k_pe_accum on the inputs of test_gpu_per_event.py's small-weight test: the phi *
gradient products (fp32, from the float64 definition) are converted per row and summed per tile coefficient, once truncating
towards zero (mpc_to_fixed) and once rounding to nearest (pe_to_fixed, what the kernel does).  The derived bound -- the accounting's
fp32 rule plus one rounding of 2^-31 per row added, times |GCOEF| max |phi| -- holds for rounding and not for truncation."""
import numpy as np
import torch

from grad_accounting import POINT_TIGHT
from oracle import focus_oracle as O


def test_rounding_to_nearest_meets_the_bound_of_one_rounding_per_row_and_truncation_does_not():
    shape, B, M, nb, k, sp = (96, 128), 2, 12000, 5, 3, 4
    hq, wq = shape[0] // sp, shape[1] // sp
    t_ref = float(np.float32(0.41))
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=31, pad_frac=0.1)
    ev[..., 5] *= 1e-4
    coeff = torch.randn(B, 1, 2 * k, *shape, generator=torch.Generator().manual_seed(8)) * 2.0
    evd = ev.double()
    c = coeff.double()[:, 0][..., O.tile_mask(shape, sp)].reshape(B, 2, k, hq, wq).permute(0, 1, 3, 4, 2)
    iy, ix = (evd[..., 0] / sp).floor().long().clamp(0, hq - 1), (evd[..., 1] / sp).floor().long().clamp(0, wq - 1)
    tr = torch.tensor([t_ref], dtype=torch.float64)
    phi = O.basis_matrix(tr, k, 'polynomial')[None] - O.basis_matrix(evd[..., 2].reshape(-1), k, 'polynomial').reshape(B, M, k)
    flow = (c[torch.arange(B)[:, None], :, iy, ix] * phi[:, :, None, :]).sum(-1)
    warped = (evd[..., :2] + flow)[:, None].clone().requires_grad_(True)
    iwes, _ = O.make_iwes(evd, warped, tr, shape, True, True, True, num_pos)
    val = O.contrast_value(iwes, 'gradient_magnitude', 'l2')
    (1 / val).backward()
    gcoef = -1.0 / float(val.detach()) ** 2 / (B * 2 * shape[0] * shape[1])          # contrast.hip, 'l2'
    g = (warped.grad[:, 0] / gcoef).float()                  # d objective / d warped position per row, as the kernel holds it
    prod = phi.float()[:, :, None, :] * g[:, :, :, None]     # [B, M, 2, k] fp32 products
    cell = (iy * wq + ix)[:, :, None].expand(B, M, 2 * k)
    valid = ev[..., 5] != 0
    n_rows = torch.zeros(B, hq * wq, dtype=torch.float64).scatter_add_(1, iy * wq + ix, valid.double())[..., None]
    phi_max = float(phi[valid].abs().max())
    want = torch.zeros(B, hq * wq, 2 * k, dtype=torch.float64).scatter_add_(1, cell, prod.double().reshape(B, M, 2 * k)) * gcoef
    allowed = POINT_TIGHT[0] * want.abs().max() + POINT_TIGHT[1] * want.abs() + n_rows * 2.0 ** -31 * abs(gcoef) * phi_max
    worst = {}
    for name, rnd in (('truncate', torch.trunc), ('nearest', torch.round)):
        hi = torch.trunc(prod)
        fixed = (hi.double() * 2 ** 30 + rnd(((prod - hi) * float(2 ** 30)).double())) / 2 ** 30
        err = torch.zeros_like(want).scatter_add_(1, cell, (fixed - prod.double()).reshape(B, M, 2 * k)) * gcoef
        worst[name] = float((err.abs() / allowed).max())
    print('worst |fixed-point error| / allowed:', worst)
    assert worst['nearest'] <= 1.0 < worst['truncate'], worst
