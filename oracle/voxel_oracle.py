"""CPU ORACLE for the voxel-grid builder -- TEST INFRASTRUCTURE ONLY.

Pure-torch restatement of reference src/loader/dsec/utils.py:29-77 (VoxelGrid.convert: trilinear
`put_(accumulate=True)` over the 8 corners, then mean/std or max normalisation of the non-zero
entries).  Pinned by tests/golden/g8_voxel_*.npz, produced by the unmodified reference
(oracle/gen_golden_voxel.py; that file of the reference imports only torch and numpy)."""
import torch


def voxel_grid(x, y, t, p, shape, norm_type='mean_std', quantile=0.0):
    """x, y, t, p: [N] float tensors (t increasing; normalised with its first and last element as in
    utils.py:35-36), shape (C, H, W).  Returns [C, H, W]."""
    C, H, W = shape
    grid = torch.zeros(C * H * W, dtype=torch.float32)
    tn = (C - 1) * (t - t[0]) / (t[-1] - t[0])
    x0, y0, t0 = x.int(), y.int(), tn.int()              # truncation, utils.py:38-40
    val = 2 * p - 1
    for xl in (x0, x0 + 1):
        for yl in (y0, y0 + 1):
            for tl in (t0, t0 + 1):
                m = (xl < W) & (xl >= 0) & (yl < H) & (yl >= 0) & (tl >= 0) & (tl < C)
                w = val * (1 - (xl - x).abs()) * (1 - (yl - y).abs()) * (1 - (tl - tn).abs())
                idx = H * W * tl.long() + W * yl.long() + xl.long()
                grid.put_(idx[m], w[m], accumulate=True)
    grid = grid.reshape(C, H, W)
    if quantile > 0:                                     # utils.py:57-61: clip at the (1 - quantile) quantile of |grid|
        thr = torch.quantile(grid.abs().view(-1), 1 - quantile)
        grid = torch.where(grid.abs() > thr, grid.sign() * thr, grid)
    if norm_type == 'mean_std':
        nz = torch.nonzero(grid, as_tuple=True)
        if nz[0].numel() > 0:
            mean, std = grid[nz].mean(), grid[nz].std()
            grid[nz] = (grid[nz] - mean) / std if std > 0 else grid[nz] - mean
    elif norm_type == 'max':
        mx = grid.abs().max()
        if mx > 0:
            grid = grid / mx
    return grid


def voxel_grid64(x, y, t, p, shape, norm_type='mean_std', quantile=0.0):
    """The same operation with every DECISION taken in fp32 as the reference takes it (t_norm, the truncations x0 / y0 / t0, the
    masks, `std > 0`) and every product, sum and statistic in float64.  The quantile's rank is the exception: pos = fp32(1 - q) *
    fp32(n - 1), its floor and its weight stay in fp32 and the at::lerp form is used -- what torch.quantile does for a float32
    input.  Returns (grid [C, H, W] float64, taps [C, H, W] int64: the taps that land on each entry, raw [C, H, W] float64: the
    grid before clipping and normalisation, m: the multiplier applied last -- 1, 1 / std or 1 / max)."""
    C, H, W = shape
    x, y, t, p = (v.float() for v in (x, y, t, p))
    grid = torch.zeros(C * H * W, dtype=torch.float64)
    taps = torch.zeros(C * H * W, dtype=torch.int64)
    if x.numel() > 0:
        tn = (C - 1) * (t - t[0]) / (t[-1] - t[0])       # fp32: it decides t0
        x0, y0, t0 = x.int(), y.int(), tn.int()
        xd, yd, td, val = x.double(), y.double(), tn.double(), 2 * p.double() - 1
        for xl in (x0, x0 + 1):
            for yl in (y0, y0 + 1):
                for tl in (t0, t0 + 1):
                    m = (xl < W) & (xl >= 0) & (yl < H) & (yl >= 0) & (tl >= 0) & (tl < C)
                    w = val * (1 - (xl - xd).abs()) * (1 - (yl - yd).abs()) * (1 - (tl - td).abs())
                    idx = H * W * tl.long() + W * yl.long() + xl.long()
                    grid.put_(idx[m], w[m], accumulate=True)
                    taps.put_(idx[m], torch.ones_like(idx[m]), accumulate=True)
    raw = grid.clone().reshape(C, H, W)
    mult = 1.0
    if quantile > 0:
        srt = torch.sort(grid.abs()).values
        pos = torch.tensor(1 - quantile, dtype=torch.float32) * torch.tensor(float(grid.numel() - 1), dtype=torch.float32)
        fl = torch.floor(pos)
        wgt = float(pos - fl)                             # (fp32 arithmetic, then widened)
        below, above = float(srt[int(fl)]), float(srt[int(torch.ceil(pos))])
        d = above - below
        thr = below + wgt * d if wgt < 0.5 else above - d * (1 - wgt)
        grid = torch.where(grid.abs() > thr, grid.sign() * thr, grid)
    if norm_type == 'mean_std':
        nz = grid != 0
        if int(nz.sum()) > 0:
            v = grid[nz]
            mean, std = v.mean(), v.std()
            if bool(v.float().std() > 0):                # the reference's decision, on its fp32 values
                grid[nz] = (v - mean) / std
                mult = 1.0 / float(std)
            else:
                grid[nz] = v - mean
    elif norm_type == 'max':
        mx = float(grid.abs().max())
        if mx > 0:
            grid = grid / mx
            mult = 1.0 / mx
    return grid.reshape(C, H, W), taps.reshape(C, H, W), raw, mult


def synth_raw_events(n, shape, seed=0, spill=2.0):
    """Seeded raw events as the DSEC slicer hands them to the voxel grid: rectified float coordinates
    that may fall slightly outside the sensor, increasing timestamps, polarity in {0, 1}."""
    g = torch.Generator().manual_seed(seed)
    C, H, W = shape
    x = torch.rand(n, generator=g) * (W - 1 + 2 * spill) - spill
    y = torch.rand(n, generator=g) * (H - 1 + 2 * spill) - spill
    t = torch.sort(torch.rand(n, generator=g)).values
    t = (t - t[0]) / (t[-1] - t[0])
    p = (torch.rand(n, generator=g) > 0.5).float()
    return x, y, t, p
