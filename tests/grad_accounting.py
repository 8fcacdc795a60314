"""Accountable gradient checks: every element that differs from the reference must be EXPLAINED (plain module imported by tests).

Two implementations of the loss can disagree on the backward for a legitimate reason only where the forward path is
discontinuous and their roundings fall on different sides:
  * sign() of the 'l1' objective at a Sobel response that is zero up to rounding (the HIP path sums the IWE in Q33.30
    integers, the oracle in fp32): every event that votes within reach of such a pixel gets a different, equally valid,
    gradient -- `near_zero_pixels`;
  * floor(pos + 1e-6) and the strict border tests (< 0, > H, > W) on the warped position, when the two LUTs the events were
    warped with differ by rounding -- `boundary_events`.
`explained_lut_cells` maps both to the LUT cells of the events concerned, `explained_points` carries the cells to trajectory
points through the oracle's actual neighbour sets, and `assert_accountable` demands that every mismatch is explained, that
mismatches are rare and that the excuse itself covers a minority of the elements.  A backward bug in a rarely taken branch
shows up as an unexplained element."""
import torch
import torch.nn.functional as F

from oracle import focus_oracle as O

LUT_TOL = 1e-5
# The stage tests hold the LUT to LUT_TOL absolute; a warped position is one fp32 add of the LUT value to the event position,
# so end to end the two positions differ by at most LUT_TOL plus one fp32 ulp of a coordinate below 1024 (2**-14 = 6.1e-5):
# 7.1e-5, rounded up.
BOUNDARY_DELTA = 1e-4
# tight rules: (fraction of the largest |want|, fraction of the element's own |want|)
LUT_TIGHT = (2e-5, 1e-4)
POINT_TIGHT = (5e-5, 2e-4)
# where only boundary events can explain (no sign() in the objective), at most this many elements may mismatch
HANDFUL = 16
# reach of a changed sign on the raw IWE: Sobel^T (1) + blur^T (1) + the folded reflect ring (1) + the bilinear tap (1)
_REACH = 9
# reach of a weight switched on or off at a tap pixel: blur (1) + Sobel (1) change the responses, Sobel^T (1) + blur^T (1) the
# adjoint image, and the other events' bilinear taps add one more
_SWITCH_REACH = 11


def _nchw(img):
    return img[:, None] if img.dim() == 3 else img


def _dilate(mask, k=_REACH):
    return F.max_pool2d(mask.float(), k, stride=1, padding=k // 2) > 0


def near_zero_pixels(blurred_iwe, rel=1e-5):
    """Pixels inside the image support whose Sobel x or y response is below `rel` times its largest magnitude, and the raw-IWE
    pixels such a sign flip can change (through Sobel^T and blur^T, 9x9 reach with the bilinear tap).  `blurred_iwe` is
    [B*T, 2, H, W] or [B*T, H, W]; both masks come back in that shape."""
    b = _nchw(blurred_iwe.detach().float().cpu())
    dx, dy = O.sobel(b)
    scale = max(dx.abs().max().item(), dy.abs().max().item())
    support = F.max_pool2d(b.abs(), 5, stride=1, padding=2) > 0
    nz = ((dx.abs() < rel * scale) | (dy.abs() < rel * scale)) & support
    aff = _dilate(nz)
    if blurred_iwe.dim() == 3:
        return nz[:, 0], aff[:, 0]
    return nz, aff


def pyramid_near_zero_pixels(raw_iwe, levels, rel=1e-5):
    """The same for the IWE pyramid (2x2 averages of the raw IWE, blur + objective on every level): a near-zero response of level
    l reaches, through its 9x9 neighbourhood on that level, the 2^l x 2^l level-0 pixels under every level-l pixel it touches.
    `raw_iwe` [N, C, H, W] -> affected level-0 pixels [N, C, H, W]."""
    cur = raw_iwe.detach().float().cpu()
    aff = torch.zeros(cur.shape, dtype=torch.bool)
    for lv in range(levels):
        _, a = near_zero_pixels(O.gaussian_blur3(cur), rel)
        s = 2 ** lv
        aff |= a.repeat_interleave(s, -2).repeat_interleave(s, -1)
        cur = F.avg_pool2d(cur, 2)
    return aff


def boundary_events(warped, shape, delta=BOUNDARY_DELTA, mask_border=True):
    """[B, T, M] bool: warped positions ([B, T, M, 2], (y, x)) within `delta` of a floor(pos + 1e-6) edge or, with the border
    mask on, of the strict border tests (y < 0, y > H, x < 0, x > W).  Only these events can change pixel or mask when the two
    LUTs differ by rounding."""
    p = warped.detach().float().cpu()
    q = p + 1e-6
    fr = q - torch.floor(q)
    hit = ((fr < delta) | (fr > 1 - delta)).any(-1)
    if mask_border:
        H, W = shape
        y, x = p[..., 0], p[..., 1]
        hit |= (y.abs() < delta) | ((y - H).abs() < delta) | (x.abs() < delta) | ((x - W).abs() < delta)
    return hit


def _taps(warped, shape):
    H, W = shape
    q = torch.floor(warped.detach().float().cpu() + 1e-6).long()
    return q[..., 0].clamp(0, H - 1), q[..., 1].clamp(0, W - 1)


def explained_lut_cells(events, warped, num_pos, shape, sp, num_bins, affected=None, boundary=None, polarity_split=True):
    """bool [B, nb, hq, wq, T]: LUT cells holding at least one event whose taps touch an `affected` pixel of its image, or that
    is one of the `boundary` events.  A boundary event at the image border also changes the image around it (the mask tests
    switch its whole weight), so its tap pixel joins the affected set, 11x11 reach.
    events [B, M, 6] in the row order the loss saw (the bucket-ordered layout permutes rows inside each polarity block: pass
    the ordered tensor), warped [B, T, M, 2]; `affected` [B*T, 2, H, W] with the polarity split by row index < num_pos, else
    [B*T, H, W]; padding rows (weight 0) explain nothing."""
    ev = events.detach().float().cpu()
    B, M, _ = ev.shape
    T = warped.shape[1]
    H, W = shape
    hq, wq = -(-H // sp), -(-W // sp)
    y0, x0 = _taps(warped, shape)                                                    # [B, T, M]
    if polarity_split:
        pol = (torch.arange(M) >= num_pos).long()[None, None].expand(B, T, M)
    else:
        pol = torch.zeros(B, T, M, dtype=torch.long)
    img = (torch.arange(B)[:, None, None] * T + torch.arange(T)[None, :, None]).expand(B, T, M)
    aff = torch.zeros(B * T, 2 if polarity_split else 1, H, W, dtype=torch.bool)
    if affected is not None:
        aff |= _nchw(affected.cpu())
    valid = (ev[..., 5] != 0)[:, None].expand(B, T, M)
    hit = torch.zeros(B, T, M, dtype=torch.bool)
    if boundary is not None:
        bnd = boundary.cpu() & valid
        # (a floor edge moves no weight -- the bilinear vote is continuous there -- but the border tests switch all of it)
        p = warped.detach().float().cpu()
        at_border = bnd & ((p[..., 0].abs() < 1e-3) | ((p[..., 0] - H).abs() < 1e-3) | (p[..., 1].abs() < 1e-3) |
                           ((p[..., 1] - W).abs() < 1e-3))
        moved = torch.zeros_like(aff)
        moved[img[at_border], pol[at_border], y0[at_border], x0[at_border]] = True
        aff |= _dilate(moved, _SWITCH_REACH)
        hit |= bnd
    hit |= aff[img, pol, y0, x0]
    hit &= valid
    it = ev[..., 4].long().clamp(0, num_bins - 1)[:, None].expand(B, T, M)
    iy = torch.div(ev[..., 0], sp, rounding_mode='floor').long().clamp(0, hq - 1)[:, None].expand(B, T, M)
    ix = torch.div(ev[..., 1], sp, rounding_mode='floor').long().clamp(0, wq - 1)[:, None].expand(B, T, M)
    r = torch.arange(T)[None, :, None].expand(B, T, M)
    bi = torch.arange(B)[:, None, None].expand(B, T, M)
    cells = torch.zeros(B, num_bins, hq, wq, T, dtype=torch.bool)
    cells[bi[hit], it[hit], iy[hit], ix[hit], r[hit]] = True
    return cells


def _scatter_points(mask_q, idx, n):
    """mask_q [B, nb, Q] over cells, idx [B, nb, Q, K] -> [B, nb, n]: the points the marked cells average."""
    B, nb, Q, K = idx.shape
    src = mask_q.float()[..., None].expand(B, nb, Q, K).reshape(B, nb, Q * K)
    out = torch.zeros(B, nb, n)
    out.scatter_add_(2, idx.reshape(B, nb, Q * K).long().cpu(), src)
    return out > 0


def explained_points(cell_mask, idx, num_points):
    """Trajectory points [B, T + nb, n] explained by `cell_mask` [B, nb, hq, wq, T] through the neighbour indices idx
    [B, nb, Q, K] (oracle.interpolate_flow(..., return_idx=True), or the device's sets where they are checked elsewhere).  Cell
    (b, t, q, r) averages traj[T + t] - traj[r] over its K neighbours: it explains those points of row T + t, and of t_ref row r.
    flow_to_next (traj[T + t + 1] - traj[T + t] over the same neighbours) needs no mapping: it feeds only the smoothness term,
    which is smooth, and no event, so nothing on that path has a discontinuity to explain."""
    B, nb, hq, wq, T = cell_mask.shape
    cm = cell_mask.reshape(B, nb, hq * wq, T).cpu()
    out = torch.zeros(B, T + nb, num_points, dtype=torch.bool)
    out[:, T:] = _scatter_points(cm.any(-1), idx, num_points)
    for r in range(T):
        out[:, r] = _scatter_points(cm[..., r], idx, num_points).any(1)
    return out


def _cell_elements(cell_mask, idx, num_points, grid):
    """[C, F] flat indices of the elements each explained cell reaches (C = explained cells): points of [B, T + nb, n], or with
    grid=True tiles of [B, n]."""
    B, nb, hq, wq, T = cell_mask.shape
    b, t, y, x, r = cell_mask.cpu().nonzero().unbind(1)
    p = idx.long().cpu()[b, t, y * wq + x]                                          # [C, K]
    if grid:
        return b[:, None] * num_points + p
    rows = T + nb
    return torch.cat(((b * rows + T + t)[:, None] * num_points + p, (b * rows + r)[:, None] * num_points + p), 1)


def _cells_needed(bad, cell_elems, limit):
    """How many explained cells it takes to account for every mismatching element: a greedy cover (an upper bound on the fewest
    that would do), stopped once it passes `limit`."""
    left = bad.reshape(-1).clone()
    n = 0
    while cell_elems.numel() and left.any() and n <= limit:
        cov = left[cell_elems].sum(1)
        best = int(cov.argmax())
        if cov[best] == 0:
            break
        left[cell_elems[best]] = False
        n += 1
    return n


def per_event_tiles(cell_mask):
    """Per-event basis warp: an event moves with the coefficients of its own tile, so a tile is explained when any of its cells
    is ([B, nb, hq, wq, T] -> [B, hq, wq])."""
    return cell_mask.any(-1).any(1)


def assert_accountable(got, want, explained, *, tight=LUT_TIGHT, max_mismatch=0.01, max_explained=0.25, excuse=None, origin=None,
                       label='', caps=True):
    """got / want: `explained.shape` or `explained.shape + (D,)` (the last axis, e.g. (y, x), is judged as one element).
    An element mismatches when |got - want| (max over the last axis) exceeds tight[0] * max|want| + tight[1] * |want|.  Asserts:
    no unexplained mismatch, mismatch fraction <= max_mismatch (1 % at most), explained fraction <= max_explained (25 % at most).
    Where elements are reached from LUT cells through their neighbours, one sign flip fans out over many elements, so both caps
    are taken where the excuse originates:
      origin = (cell_elems [C, F], number of LUT cells): the mismatch cap applies to the LUT cells it takes to account for the
               mismatching elements (_cells_needed);
      excuse (the explained LUT cells): the explained cap applies to them (K = 32 at DSEC size).
    caps=False: only 'no unexplained mismatch' is asserted here; the caller reads the two fractions from the result and must judge
    a case that passes a cap by another rule (tools/fuzz_per_event.py: images of a dozen tiles, where 1 % is less than one tile).
    Returns the counts and fractions (and prints them: pytest -s)."""
    assert max_mismatch <= 0.01 and max_explained <= 0.25
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    explained = torch.as_tensor(explained).cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.shape != explained.shape:
        assert got.shape[:-1] == explained.shape, (got.shape, explained.shape)
        err, mag = (got - want).abs().amax(-1), want.abs().amax(-1)
    else:
        err, mag = (got - want).abs(), want.abs()
    gmax = float(want.abs().max())
    assert gmax > 0, f'{label}: the reference gradient is zero'
    bad = err > tight[0] * gmax + tight[1] * mag
    unexplained = bad & ~explained
    n = bad.numel()
    res = dict(n=n, mismatch=int(bad.sum()), explained=int(explained.sum()), unexplained=int(unexplained.sum()),
               frac_mismatch=float(bad.float().mean()), frac_explained=float(explained.float().mean()),
               worst=float(err.max()) / gmax, worst_unexplained=float(err[unexplained].max()) / gmax if unexplained.any() else 0.0)
    res['frac_excuse'] = res['frac_explained'] if excuse is None else float(torch.as_tensor(excuse).float().mean())
    res['frac_mismatch_origin'] = res['frac_mismatch']
    if origin is not None and not unexplained.any():
        cell_elems, n_cells = origin
        res['mismatch_cells'] = _cells_needed(bad, cell_elems, int(max_mismatch * n_cells))
        res['frac_mismatch_origin'] = res['mismatch_cells'] / n_cells
    print(f'[accounting] {label}: {n} elements, explained {100 * res["frac_explained"]:.2f} %, mismatching '
          f'{100 * res["frac_mismatch"]:.3f} % ({res["mismatch"]}), worst {res["worst"]:.1e} of max'
          + ('' if excuse is None else f'; explained cells {100 * res["frac_excuse"]:.2f} %')
          + ('' if origin is None or unexplained.any() else
             f'; mismatching from {res["mismatch_cells"]} LUT cells ({100 * res["frac_mismatch_origin"]:.3f} %)'))
    assert res['unexplained'] == 0, (f'{label}: {res["unexplained"]} of {n} elements differ with nothing to explain them '
                                     f'({res["mismatch"]} mismatching, {res["explained"]} explained); worst unexplained '
                                     f'{res["worst_unexplained"]:.2e} of max')
    res['caps_hold'] = res['frac_mismatch_origin'] <= max_mismatch and res['frac_excuse'] <= max_explained
    if not caps:
        return res
    assert res['frac_mismatch_origin'] <= max_mismatch, (
        f'{label}: {100 * res["frac_mismatch"]:.3f} % mismatching ({res["mismatch"]} of {n})' +
        ('' if origin is None else f', from {100 * res["frac_mismatch_origin"]:.3f} % of the LUT cells'))
    assert res['frac_excuse'] <= max_explained, f'{label}: the excuse covers {100 * res["frac_excuse"]:.2f} %' + \
        (' of the elements' if excuse is None else ' of the LUT cells')
    return res


def _sign_objective(cfg):
    return cfg.get('loss_type', 'gradient_magnitude') != 'variance' and cfg['focus_loss_norm'] == 'l1'


def lut_accounting(cfg, events, num_pos, lut, got, want, *, blurred=None, label='', **kw):
    """LUT-level check (both sides warp with the same LUT, so positions agree bit for bit and only sign() can explain):
    got / want [B, nb, hq, wq, T, 2]."""
    T, sp, shape = cfg['num_tref'], cfg['lut_superpixel_size'], tuple(cfg['image_shape'])
    split = cfg['polarity_aware_batching']
    warped = O.warp_events(events.cpu(), lut.detach().cpu(), sp)
    aff = None
    if _sign_objective(cfg):
        if blurred is None:
            t_ref = kw.pop('t_ref')
            blurred, _ = O.make_iwes(events.cpu(), warped, t_ref, shape, cfg['scale_iwe_by_dt'], cfg['mask_image_border'], split,
                                     num_pos)
        _, aff = near_zero_pixels(blurred.reshape(-1, *(2,) * split, *shape))
    kw.pop('t_ref', None)
    cells = explained_lut_cells(events, warped, num_pos, shape, sp, cfg['num_bins'], aff, None, split)
    return assert_accountable(got, want, cells, tight=LUT_TIGHT, label=label, **kw)


def end_to_end_accounting(cfg, events, num_pos, traj, got, want, *, blurred=None, lut=None, idx=None, affected=None,
                          grid=False, cap_cells=False, label='', **kw):
    """Trajectory-level check of d loss / d trajectories ([B, T + nb, n, 2]) against the oracle's.  The LUT and neighbour sets
    default to the oracle's (interpolate_flow); `blurred` (the oracle's blurred IWEs) to a recomputation from them; `affected`
    replaces the near-zero set (the pyramid's).  Sign flips count only for the 'l1' gradient-magnitude objective; boundary events
    always, and where nothing else can explain, at most HANDFUL elements may mismatch.  grid=True: got / want are the gradient
    of the coefficient grid at the tile centres [B, 1, 2k, n] (a tile's coefficients move only its own trajectory, all rows).
    The 1 % mismatch cap applies to the LUT cells that account for the mismatching elements; cap_cells=True puts the 25 % cap
    on the explained LUT cells too (see assert_accountable).  Returns assert_accountable's dict plus the number of boundary
    events."""
    T, sp, shape, nb = cfg['num_tref'], cfg['lut_superpixel_size'], tuple(cfg['image_shape']), cfg['num_bins']
    split = cfg['polarity_aware_batching']
    traj = traj.detach().cpu()
    if lut is None or idx is None:
        lut, _, idx = O.interpolate_flow(traj[:, :T], traj[:, T:], shape, sp, cfg['num_knn'], cfg['dist_norm'],
                                         cfg['interpolation_scheme'], return_idx=True)
    ev = events.detach().cpu()
    warped = O.warp_events(ev, lut.detach().cpu(), sp)
    aff = affected
    if aff is None and _sign_objective(cfg):
        if blurred is None:
            blurred, _ = O.make_iwes(ev, warped, kw.pop('t_ref'), shape, cfg['scale_iwe_by_dt'], cfg['mask_image_border'], split,
                                     num_pos)
        _, aff = near_zero_pixels(blurred.reshape(-1, *(2,) * split, *shape))
    kw.pop('t_ref', None)
    bnd = boundary_events(warped, shape, mask_border=cfg['mask_image_border']) & (ev[..., 5] != 0)[:, None]
    cells = explained_lut_cells(ev, warped, num_pos, shape, sp, nb, aff, bnd, split)
    pts = explained_points(cells, idx, traj.shape[2])
    if grid:
        got, want, pts = _grid_layout(got), _grid_layout(want), pts.any(1)
    origin = (_cell_elements(cells, idx, traj.shape[2], grid), cells.numel())
    res = assert_accountable(got, want, pts, tight=POINT_TIGHT, excuse=cells if cap_cells else None, origin=origin, label=label,
                             **kw)
    res['boundary_events'] = int(bnd.sum())
    if aff is None:
        assert res['mismatch'] <= HANDFUL, f'{label}: {res["mismatch"]} elements mismatch with no sign() to explain them'
    return res


def _grid_layout(g):
    """[B, 1, 2k, n] (coefficient grid at the tile centres) -> [B, n, 2k]."""
    g = torch.as_tensor(g)
    return g.reshape(g.shape[0], -1, g.shape[-1]).transpose(1, 2)


def per_event_accounting(cfg, events, num_pos, coeff, t_ref, num_basis, basis_type, got, want, *, label='', **kw):
    """The per-event basis warp: d loss / d coefficient grid ([B, 1, 2k, H, W], compared at the tile centres) against the
    oracle's.  An event moves with the coefficients of its own tile, so a tile is explained by its own events; its positions
    are the oracle's (events + sum_k c_k (basis_k(t_ref) - basis_k(t_event))), which the device's match up to rounding."""
    sp, shape = cfg['lut_superpixel_size'], tuple(cfg['image_shape'])
    split = cfg['polarity_aware_batching']
    H, W = shape
    hq, wq = -(-H // sp), -(-W // sp)
    ev = events.detach().cpu()
    B, M, _ = ev.shape
    c = torch.as_tensor(coeff).detach().cpu()
    c = c[:, None] if c.dim() == 4 else c
    c = c.sum(1)[:, :, sp // 2::sp, sp // 2::sp]
    hc, wc = c.shape[-2:]                        # (< hq, wq where the last cells have no centre in the image: zero coefficients)
    c = F.pad(c, (0, wq - wc, 0, hq - hc)).reshape(B, 2, num_basis, hq, wq).permute(0, 1, 3, 4, 2)
    t = torch.as_tensor(t_ref, dtype=torch.float32).reshape(1)
    iy = torch.div(ev[..., 0], sp, rounding_mode='floor').long().clamp(0, hq - 1)
    ix = torch.div(ev[..., 1], sp, rounding_mode='floor').long().clamp(0, wq - 1)
    phi = O.basis_matrix(t, num_basis, basis_type)[None] - \
        O.basis_matrix(ev[..., 2].reshape(-1), num_basis, basis_type).reshape(B, M, num_basis)
    flow = (c[torch.arange(B)[:, None], :, iy, ix] * phi[:, :, None, :]).sum(-1)
    warped = (ev[..., :2] + flow)[:, None]
    aff = None
    if _sign_objective(cfg):
        blurred, _ = O.make_iwes(ev, warped, t, shape, cfg['scale_iwe_by_dt'], cfg['mask_image_border'], split, num_pos)
        _, aff = near_zero_pixels(blurred)
    bnd = boundary_events(warped, shape, mask_border=cfg['mask_image_border']) & (ev[..., 5] != 0)[:, None]
    tiles = per_event_tiles(explained_lut_cells(ev, warped, num_pos, shape, sp, cfg['num_bins'], aff, bnd, split))
    m = O.tile_mask(shape, sp)
    sel = lambda g: _grid_layout(torch.as_tensor(g).detach().cpu()[..., m])                # noqa: E731
    res = assert_accountable(sel(got), sel(want), tiles[:, :hc, :wc].reshape(B, -1), tight=POINT_TIGHT, label=label, **kw)
    res['boundary_events'] = int(bnd.sum())
    if aff is None:
        assert res['mismatch'] <= HANDFUL, f'{label}: {res["mismatch"]} elements mismatch with no sign() to explain them'
    return res
