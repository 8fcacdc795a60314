"""CPU ORACLE for the centred voxel grid -- TEST INFRASTRUCTURE ONLY.

Plain-torch restatement of reference src/loader/utils/representation.py:9-111 (VoxelGrid.convert, norm_voxel_grid) and of the
resize of src/loader/evimo2/datasubset.py:189.  Pinned by tests/golden/g12_repr_*.npz, produced by the unmodified reference
(oracle/gen_golden_repr.py; that file of the reference imports only torch)."""
import math

import torch


def extended_time_window(channels, t0_center, t1_center):
    """representation.py:35-50."""
    dt = (t1_center - t0_center) / (channels - 1)
    return math.floor(t0_center - dt), math.ceil(t1_center + dt)


def taps(x, y, pol, time, shape, t0_center=None, t1_center=None):
    """Flat indices and fp32 weights of every vote, in the reference's order of `put_` calls (representation.py:78-109)."""
    C, H, W = shape
    assert not torch.is_floating_point(time)
    c0 = time[0] if t0_center is None else t0_center                   # :78-79
    c1 = time[-1] if t1_center is None else t1_center
    tn = (time - c0) / (c1 - c0) * (C - 1)                              # :58  integer differences, fp32 quotient
    t0 = tn.floor().int()                                               # :82
    val = 2 * pol.float() - 1                                           # :83
    idx, wts = [], []
    if not torch.is_floating_point(x):                                  # :85-94
        for tl in (t0, t0 + 1):
            m = (tl >= 0) & (tl < C)
            w = val * (1 - (tl - tn).abs())
            i = H * W * tl.long() + W * y.long() + x.long()
            idx.append(i[m]); wts.append(w[m])
    else:                                                               # :96-109
        x0, y0 = x.floor().int(), y.floor().int()
        for xl in (x0, x0 + 1):
            for yl in (y0, y0 + 1):
                for tl in (t0, t0 + 1):
                    m = (xl < W) & (xl >= 0) & (yl < H) & (yl >= 0) & (tl >= 0) & (tl < C)
                    w = val * (1 - (xl - x).abs()) * (1 - (yl - y).abs()) * (1 - (tl - tn).abs())
                    i = H * W * tl.long() + W * yl.long() + xl.long()
                    idx.append(i[m]); wts.append(w[m])
    return idx, wts


def voxel_grid(x, y, pol, time, shape, t0_center=None, t1_center=None, dtype=torch.float32):
    """[N] tensors (time int64, increasing) -> raw [C, H, W].  dtype=float64 sums the same fp32 taps in double (the
    summation-order check of tests/test_repr_oracle.py)."""
    C, H, W = shape
    grid = torch.zeros(C * H * W, dtype=dtype)
    if time.numel() == 0:
        return grid.reshape(C, H, W)
    for i, w in zip(*taps(x, y, pol, time, shape, t0_center, t1_center)):
        grid.put_(i, w.to(dtype), accumulate=True)                      # sequential, like the reference's
    return grid.reshape(C, H, W)


def norm_voxel_grid(grid):
    """representation.py:9-18 (returns a new tensor)."""
    grid = grid.clone()
    nz = torch.nonzero(grid, as_tuple=True)
    if nz[0].numel() > 0:
        mean, std = grid[nz].mean(), grid[nz].std()
        grid[nz] = (grid[nz] - mean) / std if std > 0 else grid[nz] - mean
    return grid


def _src(size_in, size_out):
    """Source indices and weight of F.interpolate(mode='bilinear', align_corners=False) along one axis."""
    scale = torch.tensor(size_in, dtype=torch.float32) / size_out
    r = (scale * (torch.arange(size_out, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
    i0 = r.floor().long().clamp(max=size_in - 1)
    i1 = (i0 + 1).clamp(max=size_in - 1)
    lam = (r - i0.float()).clamp(0, 1)
    return i0, i1, lam


def resize_bilinear(grid, out_size):
    """[C, H, W] -> [C, Ho, Wo], datasubset.py:189."""
    H, W = grid.shape[-2:]
    y0, y1, ly = _src(H, out_size[0])
    x0, x1, lx = _src(W, out_size[1])
    top = (1 - lx) * grid[:, y0][:, :, x0] + lx * grid[:, y0][:, :, x1]
    bot = (1 - lx) * grid[:, y1][:, :, x0] + lx * grid[:, y1][:, :, x1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def representation(x, y, pol, time, shape, t0_center=None, t1_center=None, normalize=False, out_size=None):
    g = voxel_grid(x, y, pol, time, shape, t0_center, t1_center)
    if normalize:
        g = norm_voxel_grid(g)
    if out_size is not None:
        g = resize_bilinear(g, out_size)
    return g


def synth_int_events(n, shape, t_lo, t_hi, seed, float_xy=False):
    """Seeded events: uniform integer pixels, half of them moved onto 2 000 hot pixels (crowded voxels, as a moving edge makes
    them), sorted int64 timestamps uniform in [t_lo, t_hi], random polarity; float_xy: a uniform offset in [-0.3, 0.7), so that
    some coordinates fall outside the sensor.  The draw order is part of the contract (seeds are quoted in the tests)."""
    C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, W, (n,), generator=g, dtype=torch.int32)
    y = torch.randint(0, H, (n,), generator=g, dtype=torch.int32)
    hot = torch.randint(0, H * W, (2000,), generator=g)
    sel = torch.rand(n, generator=g) < 0.5
    hp = hot[torch.randint(0, 2000, (n,), generator=g)]
    x = torch.where(sel, (hp % W).int(), x)
    y = torch.where(sel, (hp // W).int(), y)
    t = torch.sort(torch.randint(t_lo, t_hi + 1, (n,), generator=g, dtype=torch.int64)).values
    p = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    if float_xy:
        x = x.float() + torch.rand(n, generator=g) - 0.3
        y = y.float() + torch.rand(n, generator=g) - 0.3
    return x, y, p, t
