"""The DSEC flow files on the GPU: ground-truth targets and the flow error straight from the 16-bit PNG payload, and the
benchmark's submission payload from a dense flow.

Mirrors reference src/loader/dsec/loader.py:174-180 (`Sequence.get_data_sample`: forward_flow / flow_valid),
src/utils/metrics.py:50-56 + src/utils/flow.py:18-70 (`OpticalFlowError.run`) and scripts/dsec_inference.py:33-49
(`scale_optical_flow` + `save_flow`); the numerics run in libmpcmax.so (csrc/dsec_io.hip).  The payload is [.., H, W, 3] uint16
as `imageio` returns and takes it: channel 0 = x, channel 1 = y, channel 2 = valid.  Evaluation-time operators: no gradient."""
import ctypes

import torch

from .. import _lib as C
from ..ops import _call, _ptr, _query, _require_gpu


def _payload(png16):
    """-> ([B, H, W, 3] contiguous 16-bit tensor, had a batch axis).  uint16 as it is, int16 by its bit pattern, int32 narrowed."""
    _require_gpu(png16, 'png16')
    if png16.dtype == torch.int32:
        png16 = png16.to(torch.int16)          # (keeps the low 16 bits: the values of a 16-bit PNG)
    elif png16.dtype not in (torch.uint16, torch.int16):
        raise TypeError(f'png16 must be uint16 (int16 / int32 are accepted), got {png16.dtype}')
    batched = png16.ndim == 4
    if png16.ndim not in (3, 4) or png16.shape[-1] != 3:
        raise ValueError(f'png16 must be [B, H, W, 3] or [H, W, 3], got {tuple(png16.shape)}')
    png16 = png16 if batched else png16[None]
    return png16.contiguous(), batched


def dsec_flow_targets(png16) -> dict:
    """png16 [B, H, W, 3] or [H, W, 3] uint16 (the decoded flow PNG, on the device) ->
    {'forward_flow': [B, 2, H, W] float32, 'flow_valid': [B, H, W] bool} (without B for a single image), loader.py:174-180:
    channel 0 = (png[..., 1] - 2**15) / 128, channel 1 = (png[..., 0] - 2**15) / 128, valid = png[..., 2] != 0 (`astype(bool)`,
    not the `== 1` of flow_16bit_to_float).  Exact in fp32.  One launch, no host synchronisation, capturable into a graph."""
    png, batched = _payload(png16)
    B, H, W, _ = png.shape
    flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=png.device)
    valid = torch.empty((B, H, W), dtype=torch.bool, device=png.device)
    _call('mpc_dsec_flow_decode', png.device, _ptr(png), _ptr(flow), _ptr(valid), B, H, W)
    return {'forward_flow': flow if batched else flow[0], 'flow_valid': valid if batched else valid[0]}


def dsec_flow_error(png16, flow_pred, time_scale=None) -> dict:
    """The dict of `calculate_flow_error(forward_flow, flow_pred, flow_valid, time_scale)` for the targets of `dsec_flow_targets`,
    in one pass over the payload and the prediction: no fp32 target and no mask are written.  png16 [B, H, W, 3],
    flow_pred [B, 2, H, W], time_scale [B, 1] or None.  The same arithmetic in the same order as `calculate_flow_error`."""
    png, _ = _payload(png16)
    B, H, W, _ = png.shape
    dev = png.device
    pr = flow_pred.detach().to(device=dev, dtype=torch.float32).reshape(B, 2, H, W).contiguous()
    ts = None if time_scale is None else time_scale.to(device=dev, dtype=torch.float32).reshape(B).contiguous()
    shape = C.ErrShape(B=B, H=H, W=W)
    ws = torch.empty(_query('mpc_dsec_flow_error_workspace_bytes', dev, ctypes.byref(shape)), dtype=torch.uint8, device=dev)
    out = torch.empty(5, dtype=torch.float32, device=dev)
    _call('mpc_dsec_flow_error', dev, ctypes.byref(shape), _ptr(png), _ptr(pr), _ptr(ts), _ptr(out), _ptr(ws))
    return {k: out[i] for i, k in enumerate(('EPE', '1PE', '2PE', '3PE', 'AE'))}


def dsec_flow_png16(flow, max_magnitude=60.0):
    """flow [B, 2, H, W] or [2, H, W] float32 in (y, x) order, as `flow_from_grid` / `dense_flow_from_traj` return it ->
    the benchmark's payload [B, H, W, 3] or [H, W, 3] uint16 on the device: channel 0 = x, channel 1 = y, channel 2 = 0.
    scripts/dsec_inference.py:33-49 operation by operation in fp32: mag = sqrt(u*u + v*v); where mag > max_magnitude (strict)
    u = (u / mag) * max_magnitude and likewise v, both with that magnitude; q = u * 128 + 32768 truncated to uint16.
    UNPINNED: a pixel with a NaN or infinite component gets payload 0 in both channels; a q outside [0, 65535] (only reachable with
    max_magnitude >= 256) saturates.  One launch, no host synchronisation."""
    _require_gpu(flow, 'flow')
    batched = flow.ndim == 4
    if flow.ndim not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f'flow must be [B, 2, H, W] or [2, H, W], got {tuple(flow.shape)}')
    f = flow.detach().float()
    f = (f if batched else f[None]).contiguous()
    B, _, H, W = f.shape
    png = torch.empty((B, H, W, 3), dtype=torch.uint16, device=f.device)
    _call('mpc_dsec_flow_encode', f.device, _ptr(f), float(max_magnitude), _ptr(png), B, H, W)
    return png if batched else png[0]
