"""The DEFINITION of FocusLoss.calc_per_event_basis(basis_type='table') for the tests: oracle/focus_oracle.py's
`FocusLossOracle.calc_per_event_basis` restated with a tabulated basis in place of `basis_matrix`, built from the oracle's own
`tile_mask`, `coeff_grid_to_list`, `make_iwes`, `contrast_value` and `smoothness`.  Plain torch on the CPU, fp32 or float64 (the
dtype of the events), autograd gives the gradients w.r.t. the coefficients and the table.  The reference has no such path: the
issue's text is the specification, and `table_basis` below is its five lines."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import focus_oracle as O


def table_basis(table, times):
    """table [S + 1, k], times [...] -> [..., k]: knot i at i / S, linear in between, one operation per line."""
    S = table.shape[0] - 1
    tc = torch.clamp(torch.clamp(times, min=0.0), max=1.0)
    x = tc * float(S)
    i = torch.clamp(torch.floor(x).to(torch.int64), max=S - 1)       # t == 1 lands in the last interval with f == 1
    f = x - i.to(times.dtype)
    lo, hi = table[i], table[i + 1]
    return lo + f[..., None] * (hi - lo)


def table_basis_np64(table, times):
    """The same in numpy float64 (for the host test of utils.table_basis_values)."""
    T = np.asarray(table, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64)
    S = T.shape[0] - 1
    x = np.minimum(np.maximum(t, 0.0), 1.0) * S
    i = np.minimum(np.floor(x).astype(np.int64), S - 1)
    f = x - i
    return T[i] + f[..., None] * (T[i + 1] - T[i])


def calc_per_event_table(cfg, coeff_grid, table, t_ref, batch):
    """-> (loss, iwes): `cfg` the keyword dictionary of FocusLossOracle; everything in the dtype of batch['events']."""
    orc = O.FocusLossOracle(**cfg)
    events = batch['events']
    num_pos = batch['num_pos_events'] if 'num_pos_events' in batch else -1
    k = table.shape[1]
    h, w = orc.image_shape
    sp = orc.sp
    mask = O.tile_mask((h, w), sp)
    if coeff_grid.dim() == 4:
        coeff_grid = coeff_grid[:, None]
    coeffs, _ = O.coeff_grid_to_list(coeff_grid, mask, k)                       # [b, s, 2, n, k]
    hq, wq = -(-h // sp), -(-w // sp)
    hc, wc = len(range(sp // 2, h, sp)), len(range(sp // 2, w, sp))
    b, m, _ = events.shape
    c = coeffs.sum(1).reshape(b, 2, hc, wc, k)
    if (hc, wc) != (hq, wq):
        c = F.pad(c, (0, 0, 0, wq - wc, 0, hq - hc))
    t_ref = torch.as_tensor(t_ref, dtype=events.dtype).reshape(1)
    ib = torch.arange(b)[:, None].expand(b, m)
    iy = torch.div(events[..., 0], sp, rounding_mode='floor').to(torch.int64).clamp(0, hq - 1)
    ix = torch.div(events[..., 1], sp, rounding_mode='floor').to(torch.int64).clamp(0, wq - 1)
    phi = table_basis(table, t_ref)[None] - table_basis(table, events[..., 2].reshape(-1)).reshape(b, m, k)
    flow = (c[ib, :, iy, ix] * phi[:, :, None, :]).sum(-1)
    warped = (events[..., :2] + flow)[:, None]
    iwes, _ = O.make_iwes(events, warped, t_ref, orc.image_shape, orc.scale_iwe_by_dt, orc.mask_image_border,
                          orc.polarity_aware_batching, num_pos)
    focus = 1 / O.contrast_value(iwes, orc.loss_type, orc.focus_loss_norm)
    smooth = torch.zeros((), dtype=events.dtype)
    if orc.smooth_weight > 0:
        phim = table_basis(table, t_ref) - table_basis(table, O.bin_mid_times(orc.num_bins).to(t_ref.dtype))
        field = torch.einsum('bdhwk,tk->btdhw', c, phim).reshape(-1, 2, hq, wq)
        smooth = orc.smooth_weight * O.smoothness(field)
    return focus + smooth, iwes.detach()


def definition(cfg, ev, num_pos, coeff, table, t_ref, dtype=torch.float32, table_fn=None):
    """Loss, IWEs and the two gradients of the definition in `dtype`.  `table_fn(dtype) -> (table, parameters)` builds the table
    inside the graph (a network at the knots); then the third gradient is that of the parameters, flattened."""
    co = coeff.to(dtype).clone().requires_grad_(True)
    params = None
    if table_fn is not None:
        tb, params = table_fn(dtype)
    else:
        tb = table.to(dtype).clone().requires_grad_(True)
    t = float(np.float32(t_ref))
    loss, iwes = calc_per_event_table(cfg, co, tb, t, {'events': ev.to(dtype), 'num_pos_events': num_pos})
    if params is not None:
        gs = torch.autograd.grad(loss, [co] + list(params))
        return loss.detach(), iwes, gs[0], torch.cat([g.reshape(-1) for g in gs[1:]])
    loss.backward()
    return loss.detach(), iwes, co.grad, tb.grad


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
