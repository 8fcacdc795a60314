"""Centred voxel grid on the GPU: the network input of the EVIMO2 and MultiFlow configurations.

Mirrors reference src/loader/utils/representation.py:9-111 (`VoxelGrid(channels, height, width).convert(x, y, pol, time,
t0_center, t1_center)`, `norm_voxel_grid`) and adds the batched entry point `representation_grids`, which also applies the
normalisation and the resize of src/loader/evimo2/datasubset.py:162-189 in the same library call; the numerics run in
libmpcmax.so (csrc/repr.hip).  This is NOT the DSEC builder `utils.VoxelGrid` (utils/voxel_grid.py): integer timestamps with
caller-given centres, floor instead of truncation, a two-tap path for integer coordinates, votes of events outside the centres."""
import ctypes
import math
from typing import Optional

import torch

from .. import _lib as C
from ..ops import _call, _ptr, _query, _require_gpu


def _is_int_tensor(t: torch.Tensor) -> bool:
    return not torch.is_floating_point(t) and not torch.is_complex(t)


def _as(t: torch.Tensor, dtype) -> torch.Tensor:
    return t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()


def representation_grids(x, y, pol, time, counts, channels, height, width, centres=None, normalize=False, out_size=None,
                         downsample=False, int_xy=None) -> torch.Tensor:
    """x, y, pol, time [B, N] (padded), counts [B] valid rows per sample -> [B, C, H', W'] in one library call.

    `time` must be an integer tensor (increasing per sample).  Integer `x` (then `y` too) selects the two-tap path of
    representation.py:85-94, floating `x` the eight-tap path; `int_xy=True` selects the two-tap path for floating tensors that hold
    integers (fp32 coordinates already in the ABI's dtype: no conversion pass; an event whose coordinate is not an integer is then
    dropped).  Events outside the sensor are dropped (the reference's integer path does no bounds check: its flat index wraps or
    raises).  `centres`: None (first and last valid timestamp of each sample,
    read on the device), a pair of ints, or a [B, 2] integer tensor (its rows are not checked for t1 > t0, which would need a
    host read: t1 == t0 gives a zero grid for that sample, t1 < t0 a mirrored time axis).  `normalize`: norm_voxel_grid per sample.  `out_size`
    (Ho, Wo): F.interpolate(..., mode='bilinear', align_corners=False) after the normalisation (the EVIMO2 order).  A sample with
    counts[b] == 0 gives zeros.  Inputs that already are fp32 (x, y, pol) / int64 (time, centres) / int32 (counts), contiguous
    and on the device are passed through; anything else is converted with torch first (one extra pass per tensor).
    No host synchronisation when counts is a device tensor and centres is None, a pair or a device tensor; the call can be
    captured into a graph.
    Scratch memory: a workspace of about 260 bytes per padded event row (B x N) is taken with torch.empty on every call (buckets of
    four times the mean fill, plus worst-case spill regions and their chunk lists; 2.3 GB at 6 x 1 500 000 events) and returned to
    torch's caching allocator afterwards; mpc_repr_workspace_bytes gives the exact figure."""
    if downsample:
        raise NotImplementedError("MultiFlow's `downsample` (sample.py:108-113: halving with align_corners=True BEFORE the "
                                  'normalisation) is off in every shipped configuration and is not built')
    for name, t in (('x', x), ('y', y), ('pol', pol), ('time', time)):
        _require_gpu(t, name)
    if not (x.shape == y.shape == pol.shape == time.shape) or x.ndim != 2:
        raise ValueError(f'x, y, pol, time must share one [B, N] shape (got {tuple(x.shape)}, {tuple(y.shape)}, '
                         f'{tuple(pol.shape)}, {tuple(time.shape)})')
    if not _is_int_tensor(time):
        raise TypeError(f'time must be an integer tensor (representation.py:69), got {time.dtype}')
    if _is_int_tensor(x) and not _is_int_tensor(y):
        raise TypeError('integer x needs integer y (representation.py:72-73)')
    if int_xy is None:
        int_xy = _is_int_tensor(x)                                    # representation.py:71
    elif not int_xy and _is_int_tensor(x):
        raise ValueError('integer x, y take the two-tap path (representation.py:85)')
    channels, height, width = int(channels), int(height), int(width)
    if not (channels > 1 and height > 1 and width > 1):
        raise ValueError('channels, height and width must exceed 1 (representation.py:28-30)')
    dev = x.device
    B, N = x.shape
    if counts.ndim != 1 or counts.shape[0] != B:
        raise ValueError(f'counts must be [B] = [{B}], got {tuple(counts.shape)}')
    xf, yf, pf, tt = _as(x, torch.float32), _as(y, torch.float32), _as(pol, torch.float32), _as(time, torch.int64)
    cnt = _as(counts.to(dev), torch.int32)
    cen = None
    if centres is not None:
        if isinstance(centres, torch.Tensor):
            if centres.shape != (B, 2) or not _is_int_tensor(centres):
                raise ValueError(f'centres must be an integer [B, 2] tensor, got {tuple(centres.shape)} {centres.dtype}')
            cen = _as(centres.to(dev), torch.int64)
        else:
            c0, c1 = (int(v) for v in centres)
            if not c1 > c0:
                raise ValueError(f'centres need t1_center > t0_center (representation.py:49), got {c0}, {c1}')
            cen = torch.empty((B, 2), dtype=torch.int64, device=dev)          # two fill kernels: no staging copy from the host
            cen[:, 0] = c0
            cen[:, 1] = c1
    Ho, Wo = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if out_size is not None and (Ho < 1 or Wo < 1):
        raise ValueError(f'out_size must be positive, got {out_size}')
    shape = C.ReprShape(B=B, N=N, C=channels, H=height, W=width, int_xy=int(int_xy), norm=int(bool(normalize)), Ho=Ho, Wo=Wo)
    ws = torch.empty(max(_query('mpc_repr_workspace_bytes', dev, ctypes.byref(shape)), 256), dtype=torch.uint8, device=dev)
    grid = torch.empty((B, channels, Ho or height, Wo or width), dtype=torch.float32, device=dev)
    _call('mpc_repr_grid', dev, ctypes.byref(shape), _ptr(xf), _ptr(yf), _ptr(tt), _ptr(pf), _ptr(cnt), _ptr(cen), _ptr(grid), _ptr(ws))
    return grid


def norm_voxel_grid(voxel_grid: torch.Tensor) -> torch.Tensor:
    """representation.py:9-18 for a [C, H, W] grid on the device, in place (the reference writes into its argument too);
    returns it.  Two reductions and one update on the current stream, no host synchronisation."""
    _require_gpu(voxel_grid, 'voxel_grid')
    if voxel_grid.dtype != torch.float32 or not voxel_grid.is_contiguous():
        raise ValueError('voxel_grid must be a contiguous fp32 tensor (it is normalised in place)')
    dev = voxel_grid.device
    ws = torch.empty(max(_query('mpc_repr_norm_workspace_bytes', dev, 1), 256), dtype=torch.uint8, device=dev)
    _call('mpc_repr_norm', dev, _ptr(voxel_grid), 1, voxel_grid.numel(), _ptr(ws))
    return voxel_grid


class VoxelGrid:
    """Same constructor, `get_extended_time_window` and `convert` contract as the reference class (representation.py:26-111),
    for tensors on the GPU."""

    def __init__(self, channels: int, height: int, width: int):
        assert channels > 1
        assert height > 1
        assert width > 1
        self.nb_channels = channels
        self.height = height
        self.width = width

    def _get_dt(self, t0_center: int, t1_center: int):
        assert t1_center > t0_center
        return (t1_center - t0_center) / (self.nb_channels - 1)

    def get_extended_time_window(self, t0_center: int, t1_center: int):
        """representation.py:35-39: the window whose events vote into the first and last channel from outside the centres."""
        dt = self._get_dt(t0_center, t1_center)
        return math.floor(t0_center - dt), math.ceil(t1_center + dt)

    def convert(self, x: torch.Tensor, y: torch.Tensor, pol: torch.Tensor, time: torch.Tensor,
                t0_center: Optional[int] = None, t1_center: Optional[int] = None) -> torch.Tensor:
        """[N] tensors on the GPU -> [C, H, W].  An empty sample needs explicit centres, as in the reference."""
        for name, t in (('x', x), ('y', y), ('pol', pol), ('time', time)):
            _require_gpu(t, name)
        assert type(t0_center) == type(t1_center)
        if not (x.shape == y.shape == pol.shape == time.shape) or x.ndim != 1:
            raise ValueError('x, y, pol, time must be [N] tensors of one length')
        if time.numel() == 0 and t0_center is None:
            raise IndexError('an empty sample has no default centres (representation.py:78)')
        centres = None if t0_center is None else (int(t0_center), int(t1_center))
        cnt = torch.full((1,), time.numel(), dtype=torch.int32, device=x.device)
        with torch.no_grad():
            return representation_grids(x[None], y[None], pol[None], time[None], cnt, self.nb_channels, self.height, self.width,
                                        centres=centres)[0]
