"""Ground-truth flow targets on the GPU: the raw multi-step flow of the EVIMO2 / MultiFlow configurations -> the `flow_gt` and
`flow_valid` that `trajectory_val_metrics` takes, as the reference's loaders prepare them on the CPU (EVIMO2:
src/loader/evimo2/datasubset.py:171-188 -- NaN mask, NaN -> 0, bilinear resize, per-axis scale, nearest resize of the validity and
of the object-id mask; MultiFlow: src/loader/multiflow/sample.py:108-139 with downsample=True -- channels-last read, bilinear
resize with align_corners=True, / 2).  One launch in libmpcmax.so (csrc/flow_targets.hip: mpc_flow_targets); forward only:
ground truth carries no gradient."""
import ctypes

import torch

from .. import _lib as C
from ..ops import _call, _ptr, _require_gpu
from .ingest import _c


def flow_targets(raw_flow, out_size=None, *, dataset, id_mask=None):
    """raw_flow -> {'flow': [B, S, 2, Ho, Wo] float32, 'flow_valid': [B, S, Ho, Wo] torch.bool or None,
    'id_mask': [B, Ho, Wo] float32 or None, 'x_scale': float, 'y_scale': float}.

    dataset='evimo2': raw_flow [B, S, 2, H, W], channel order (x, y), NaN marks an invalid pixel; out_size=(Ho, Wo) is required
        ((H, W) itself is allowed); id_mask [B, H, W], optional (any dtype; converted to fp32 with torch).
        flow_valid = neither channel NaN, picked by F.interpolate(mode='nearest'); every NaN element becomes 0 on its own (a pixel
        with one NaN channel keeps the other channel's value in the blend); flow = F.interpolate(mode='bilinear',
        align_corners=False) of the zeroed field, channel 0 times fp32(Wo / W) and channel 1 times fp32(Ho / H); id_mask by the
        same nearest pick, as fp32 (the reference's .squeeze() at one sample is the collate's business).
        x_scale = Wo / W, y_scale = Ho / H: the loader's X_SCALE / Y_SCALE, what `ingest_raw_events(xy_scale=...)` takes.
    dataset='multiflow': raw_flow [B, S, H, W, 2], channels last as the h5 files store it; out_size None or (H // 2, W // 2);
        id_mask is rejected.  flow = F.interpolate(mode='bilinear', align_corners=True) / 2; no NaN treatment (a NaN propagates as
        in the reference) and no validity: flow_valid is None; x_scale = y_scale = 0.5.
    'flow' and 'flow_valid' go into `trajectory_val_metrics(flow_gt=..., flow_valid=...)` unchanged.  Other dtypes than float32 are
    converted with torch on the device first; CPU tensors raise.  Nothing synchronises the host; the call can be captured into a
    graph."""
    if dataset not in ('evimo2', 'multiflow'):
        raise ValueError(f"dataset must be 'evimo2' or 'multiflow', got {dataset!r}")
    evimo2 = dataset == 'evimo2'
    if raw_flow.ndim != 5:
        raise ValueError('raw_flow must be ' + ('[B, S, 2, H, W]' if evimo2 else '[B, S, H, W, 2]') + f', got {tuple(raw_flow.shape)}')
    if evimo2:
        B, S, ch, H, W = raw_flow.shape
        if out_size is None:
            raise ValueError("dataset='evimo2' needs out_size=(Ho, Wo) (EVIMO2_Datasubset's resize_height, resize_width)")
    else:
        B, S, H, W, ch = raw_flow.shape
        if id_mask is not None:
            raise ValueError("dataset='multiflow' has no object-id mask")
        if out_size is None:
            out_size = (H // 2, W // 2)
    if ch != 2:
        raise ValueError('raw_flow must be ' + ('[B, S, 2, H, W]' if evimo2 else '[B, S, H, W, 2]') + f', got {tuple(raw_flow.shape)}')
    if len(out_size) != 2:
        raise ValueError(f'out_size must be (Ho, Wo), got {out_size!r}')
    Ho, Wo = int(out_size[0]), int(out_size[1])
    if not evimo2 and (Ho, Wo) != (H // 2, W // 2):
        raise ValueError(f"dataset='multiflow' halves the image (sample.py:113): out_size must be {(H // 2, W // 2)}, got {(Ho, Wo)}")
    if id_mask is not None and tuple(id_mask.shape) != (B, H, W):
        raise ValueError(f'id_mask must be [B, H, W] = {(B, H, W)}, got {tuple(id_mask.shape)}')
    shape = C.TargetsShape(B=B, S=S, H=H, W=W, Ho=Ho, Wo=Wo, mode=C.TARGETS_EVIMO2 if evimo2 else C.TARGETS_MULTIFLOW,
                           has_id=int(id_mask is not None))
    if C.lib().mpc_flow_targets_supported(ctypes.byref(shape)) != 0:
        raise ValueError(C.lib().mpc_last_error_string().decode(errors='replace'))
    _require_gpu(raw_flow, 'raw_flow')
    if id_mask is not None:
        _require_gpu(id_mask, 'id_mask')
    # ---- nothing above touched the GPU
    dev = raw_flow.device
    raw = _c(raw_flow.detach(), torch.float32)
    ids = None if id_mask is None else _c(id_mask.detach(), torch.float32)
    flow = torch.empty((B, S, 2, Ho, Wo), dtype=torch.float32, device=dev)
    valid = torch.empty((B, S, Ho, Wo), dtype=torch.bool, device=dev) if evimo2 else None
    id_out = None if ids is None else torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev)
    _call('mpc_flow_targets', dev, ctypes.byref(shape), _ptr(raw), _ptr(ids), _ptr(flow), _ptr(valid), _ptr(id_out))
    return {'flow': flow, 'flow_valid': valid, 'id_mask': id_out,
            'x_scale': Wo / W if evimo2 else 0.5, 'y_scale': Ho / H if evimo2 else 0.5}
