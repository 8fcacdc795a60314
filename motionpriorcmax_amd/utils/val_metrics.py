"""The flow metrics of the RAFT-spline validation step on the GPU: what `RAFTSplineModule.validation_step` logs (reference
src/modules/raft_spline.py:88-215) -- EPE, AE, NPE(1/2/3), EPE_MULTI, AE_MULTI and FLOW_METRICS_MULTI of src/modules/utils.py:85-296,
335-541 in their unmasked, event-masked and validity-masked variants, and the linear-motion baseline (:67-74) -- as one fused
reduction in libmpcmax.so (csrc/val_metrics.hip: mpc_val_metrics).  The curves are evaluated in registers, ground truth, validity
masks and the event representation are read once, the predictions are never written and the host is never asked anything.
Evaluation-time operators: no gradient."""
import ctypes

import numpy as np
import torch

from .. import _lib as C
from ..ops import _call, _f32c, _ptr, _query, _require_gpu
from .basis import curve_basis


def val_metric_keys(num_steps):
    """The logged names in the key order of mpc_val_metrics: [(name, index into values / updated)] (45 names for six steps)."""
    M = int(num_steps)
    keys = [('val/' + k, C.VAL_SINGLE + i) for i, k in enumerate(C.VAL_SINGLE_KEYS)]
    keys += [('val/masked_' + k, C.VAL_MASKED_SINGLE + i) for i, k in enumerate(C.VAL_SINGLE_KEYS)]
    for prefix, base in (('val/', C.VAL_MULTI), ('val/ev_masked_', C.VAL_EV_MASKED_MULTI), ('val/masked_', C.VAL_MASKED_MULTI)):
        keys += [(prefix + k, base + i) for i, k in enumerate(C.VAL_MULTI_KEYS)]
        keys += [(f'{prefix}EPE_STEP{str(m).zfill(2)}', base + len(C.VAL_MULTI_KEYS) + m) for m in range(M)]
    return keys + [('val/epe_multi_lin', C.VAL_EPE_MULTI_LIN), ('val/ae_multi_lin', C.VAL_AE_MULTI_LIN)]


def _bool_bytes(t):
    if t is None:
        return None
    t = t.detach()
    return (t if t.dtype == torch.bool else t != 0).contiguous()


def _val_metrics_raw(flow_gt, timestamps, params, up_mask, scale, flows, flow_valid, ev_repr, event_mask, curve_type='BEZIER',
                     basis_network=None, scalar_time_shortcuts=True):
    """Argument checks (all before the first GPU call), then the library call: (values [75] fp32, updated [75] int32, M)."""
    if (params is None) == (flows is None):
        raise ValueError('exactly one prediction source: params (+ up_mask) or flows')
    if params is None and up_mask is not None:
        raise ValueError('up_mask goes with params')
    if (ev_repr is None) == (event_mask is None):
        raise ValueError('exactly one of ev_repr / event_mask')
    if curve_type not in ('BEZIER', 'POLYNOMIAL', 'LEARNED') or (curve_type == 'LEARNED' and basis_network is None and params is not None):
        raise ValueError(f"curve_type must be 'BEZIER', 'POLYNOMIAL' or 'LEARNED' (with basis_network), got {curve_type!r}")
    if isinstance(flow_gt, (list, tuple)):
        M = len(flow_gt)
        gt_shape = (flow_gt[0].shape[0], M) + tuple(flow_gt[0].shape[1:]) if M else ()
    else:
        gt_shape = tuple(flow_gt.shape)
        M = gt_shape[1] if len(gt_shape) == 5 else -1
    if len(gt_shape) != 5 or gt_shape[2] != 2:
        raise ValueError(f'flow_gt must be [B, M, 2, H, W] or a list of M [B, 2, H, W], got {gt_shape}')
    B, _, _, H, W = gt_shape
    n_ts = int(timestamps.numel()) if torch.is_tensor(timestamps) else int(np.asarray(timestamps).size)
    if n_ts != M:
        raise ValueError(f'{n_ts} timestamps for {M} ground-truth steps')
    if M < 1 or M > C.VAL_MAX_STEPS:
        raise ValueError(f'1 <= M <= {C.VAL_MAX_STEPS} steps, got {M}')
    d = h = w = 0
    if params is not None:
        if params.dim() != 4 or params.shape[1] % 2:
            raise ValueError(f'params must be [B, 2d, h, w], got {tuple(params.shape)}')
        d, h, w = params.shape[1] // 2, params.shape[2], params.shape[3]
        if up_mask is None or tuple(up_mask.shape) != (B, 576, h, w) or params.shape[0] != B:
            raise ValueError(f'up_mask must be [B, 576, h, w] = {(B, 576, h, w)}, got {None if up_mask is None else tuple(up_mask.shape)}')
        if (H, W) != (8 * h, 8 * w):
            raise ValueError(f'with params + up_mask the ground truth must be 8 x the grid of params: {(8 * h, 8 * w)}, got {(H, W)}')
        if d < 1 or d > 16:
            raise ValueError(f'1 <= d <= 16 control points per axis, got {d}')
    elif tuple(flows.shape) != (M, B, 2, H, W):
        raise ValueError(f'flows must be [M, B, 2, H, W] = {(M, B, 2, H, W)}, got {tuple(flows.shape)}')
    if isinstance(flow_valid, (list, tuple)):
        flow_valid = torch.stack(list(flow_valid), dim=1)
    for t, shp, name in ((flow_valid, (B, M, H, W), 'flow_valid'), (event_mask, (B, H, W), 'event_mask')):
        if t is not None and tuple(t.shape) != shp:
            raise ValueError(f'{name} must be {shp}, got {tuple(t.shape)}')
    if ev_repr is not None and (ev_repr.dim() != 4 or ev_repr.shape[0] != B or tuple(ev_repr.shape[2:]) != (H, W) or ev_repr.shape[1] < 1):
        raise ValueError(f'ev_repr must be [B, C, H, W] with B, H, W = {(B, H, W)}, got {tuple(ev_repr.shape)}')
    first = flow_gt[0] if isinstance(flow_gt, (list, tuple)) else flow_gt
    for t, name in ((first, 'flow_gt'), (params, 'params'), (up_mask, 'up_mask'), (flows, 'flows'), (flow_valid, 'flow_valid'),
                    (ev_repr, 'ev_repr'), (event_mask, 'event_mask')):
        if t is not None:
            _require_gpu(t, name)
    dev = first.device
    # ---- nothing above touched the GPU
    gt = torch.stack([g.detach() for g in flow_gt], dim=1) if isinstance(flow_gt, (list, tuple)) else flow_gt.detach()
    gt = _f32c(gt)
    flow_valid, event_mask = _bool_bytes(flow_valid), _bool_bytes(event_mask)
    if ev_repr is not None:
        ev_repr = _f32c(ev_repr.detach())
    values = torch.full((C.VAL_COUNT,), float('nan'), dtype=torch.float32, device=dev) if B == 0 else torch.empty(C.VAL_COUNT, dtype=torch.float32, device=dev)
    updated = torch.zeros(C.VAL_COUNT, dtype=torch.int32, device=dev) if B == 0 else torch.empty(C.VAL_COUNT, dtype=torch.int32, device=dev)
    if B == 0:
        return values, updated, M
    bm = None
    if params is not None:
        with torch.no_grad():                    # [M, d]; 'BEZIER': float64 on the host, then fp32 -- the cached matrix
            bm = _f32c(curve_basis(curve_type, timestamps, int(d), basis_network, scalar_time_shortcuts=scalar_time_shortcuts, device=dev))
        params, up_mask = _f32c(params.detach()), _f32c(up_mask.detach())
    else:
        flows = _f32c(flows.detach())
    if torch.is_tensor(timestamps):
        ts = timestamps.detach().to(device=dev, dtype=torch.float32).reshape(M).contiguous()
    else:
        ts = torch.tensor(np.asarray(timestamps, dtype=np.float64).reshape(M), dtype=torch.float32).to(dev)
    shape = C.ValShape(B=B, M=M, d=d, h=h, w=w, H=H, W=W, C=0 if ev_repr is None else int(ev_repr.shape[1]))
    ws = torch.empty(_query('mpc_val_metrics_workspace_bytes', dev, ctypes.byref(shape)), dtype=torch.uint8, device=dev)
    _call('mpc_val_metrics', dev, ctypes.byref(shape), _ptr(params), _ptr(up_mask), _ptr(bm), _ptr(flows), float(scale), _ptr(ts),
          _ptr(gt), _ptr(flow_valid), _ptr(ev_repr), _ptr(event_mask), _ptr(values), _ptr(updated), _ptr(ws))
    return values, updated, M


def trajectory_val_metrics(flow_gt, timestamps, *, params=None, up_mask=None, scale=1.0, flows=None, flow_valid=None, ev_repr=None,
                           event_mask=None, curve_type='BEZIER', basis_network=None, scalar_time_shortcuts=True):
    """Every scalar `RAFTSplineModule.validation_step` logs for one batch (reference src/modules/raft_spline.py:159-194), as
    (values, updated): two dicts over the same keys, a 0-dim fp32 and a 0-dim int32 device tensor each.

    flow_gt     [B, M, 2, H, W] or a list of M [B, 2, H, W], (x, y) order, finite (the loaders zero NaN); 1 <= M <= 16
    timestamps  M times in [0, 1] (tensor, list or array): where the curves are evaluated, and -- rounded to fp32 -- the factors of
                the linear-motion baseline timestamps[m] * prediction[M - 1] (utils.py:67-74)
    predictions, exactly one of (ValueError otherwise)
      params [B, 2d, h, w] + up_mask [B, 576, h, w]: the curves of `BezierCurves(params).create_upsampled(up_mask)` evaluated inside
                the kernel (H x W = 8h x 8w; the device functions of `flows_from_bezier`: the same bits), d <= 16
      flows  [M, B, 2, H, W]: any curve type, any H x W, padded or unpadded outputs
      both times `scale`
    curve_type, basis_network, scalar_time_shortcuts (with params): the curve type of `utils.curve_basis` -- 'BEZIER' (default),
                'POLYNOMIAL' or 'LEARNED' with its basis network; only the [M, d] matrix handed to the kernel differs.
                `scalar_time_shortcuts` defaults to True HERE, and here alone: `validation_step` evaluates the curve once per SCALAR
                timestamp (raft_spline.py:134-154), and `get_flow_from_reference` answers a scalar 1 with the last control point
                and a scalar 0 with zeros whatever the curve type (curves/base.py:98-106) -- for polynomial and learned curves that
                is not the value of the basis at those times.  False evaluates every timestamp as the list call does.
    flow_valid  [B, M, H, W] bool (or a list of M [B, H, W]), optional: V_m
    ev_repr [B, C, H, W] (E = any channel != 0, a NaN counts: raft_spline.py:164) or event_mask [B, H, W] bool: exactly one

    Keys (45 for M = 6): 'val/' + epe ae 1pe 2pe 3pe (no mask, step M - 1); 'val/masked_' + the same five (mask E); for the prefixes
    'val/' (no mask), 'val/ev_masked_' (E & V_m; E alone without flow_valid) and 'val/masked_' (V_m; no mask without flow_valid)
    epe_multi ae_multi T3PE TEPE TAE EPE_STEP00 .. EPE_STEP{M-1}; 'val/epe_multi_lin', 'val/ae_multi_lin'.  The formulas are
    written out in include/mpcmax.h.  The reference's FLOW_METRICS_MULTI asserts M == 6; other M follow the functions it calls.

    updated[key] is 1 where the reference's `Metric.update` would have added the value, and 0 where it skips (the epe family when
    every mask is empty; the value is NaN) or raises (`NPE` with an empty mask, utils.py:199: all five singles of that mask are
    NaN / 0 -- this row is UNPINNED, the reference has no value there).  A NaN the reference would add (ae over an empty mask) comes
    with updated = 1.  Nothing synchronises the host.  CPU tensors raise; inputs are detached."""
    values, updated, M = _val_metrics_raw(flow_gt, timestamps, params, up_mask, scale, flows, flow_valid, ev_repr, event_mask,
                                          curve_type, basis_network, scalar_time_shortcuts)
    keys = val_metric_keys(M)
    return {k: values[i] for k, i in keys}, {k: updated[i] for k, i in keys}


class TrajectoryValMetrics:
    """The epoch accumulator over `trajectory_val_metrics`: the counterpart of the reference's Metric objects (utils.py:335-541) for
    all keys at once.  `update(**same arguments)` (curve_type / basis_network / scalar_time_shortcuts included) adds every value
    whose `updated` flag is set to an fp64 sum and the flag to an int64
    total, on the device and without a host synchronisation; `compute()` returns sum / total per key as fp32 (`Metric.compute`; a key
    never updated gives NaN where the reference asserts); `state()` returns the two device tensors (sums [75] fp64, totals [75]
    int64) themselves, to be summed across ranks in place (all_reduce) -- the counterpart of dist_reduce_fx="sum".
    All sums are held in fp64: the reference keeps the FLOW_METRICS_MULTI states (T3PE, TEPE, TAE, EPE_STEPmm) in fp32 and the others
    in fp64.  A NaN the reference would add is added."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = self._totals = None
        self._steps = 0

    def update(self, flow_gt, timestamps, **kwargs):
        values, updated, M = _val_metrics_raw(flow_gt, timestamps, kwargs.pop('params', None), kwargs.pop('up_mask', None),
                                              kwargs.pop('scale', 1.0), kwargs.pop('flows', None), kwargs.pop('flow_valid', None),
                                              kwargs.pop('ev_repr', None), kwargs.pop('event_mask', None),
                                              kwargs.pop('curve_type', 'BEZIER'), kwargs.pop('basis_network', None),
                                              kwargs.pop('scalar_time_shortcuts', True))
        if kwargs:
            raise TypeError(f'unexpected arguments {sorted(kwargs)}')
        if self._sums is None:
            self._sums = torch.zeros(C.VAL_COUNT, dtype=torch.float64, device=values.device)
            self._totals = torch.zeros(C.VAL_COUNT, dtype=torch.int64, device=values.device)
        elif M != self._steps:
            raise ValueError(f'{M} steps after batches of {self._steps}')
        self._steps = M
        self._sums += torch.where(updated != 0, values.double(), torch.zeros((), dtype=torch.float64, device=values.device))
        self._totals += updated

    def state(self):
        if self._sums is None:
            raise RuntimeError('no batch yet')
        return self._sums, self._totals

    def compute(self):
        sums, totals = self.state()
        out = (sums / totals.double()).float()
        return {k: out[i] for k, i in val_metric_keys(self._steps)}
