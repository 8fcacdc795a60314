"""Event ingest on the GPU: raw windows -> the padded [B, M, 6] event tensor and
`num_pos_events` that `FocusLoss.calc` consumes, and (optionally) the (x, y, t, p) rows for the
voxel-grid builder.  `ingest_events` mirrors reference src/loader/dsec/loader.py:152-167 + 360-415,
`ingest_raw_events` the EVIMO2 and MultiFlow loaders (src/loader/evimo2/datasubset.py:206-228,
src/loader/multiflow/sample.py:224-236) with the collate of src/modules/data_loading.py:14-47; numerics in
libmpcmax.so (csrc/ingest.hip)."""
import ctypes

import torch

from .. import _lib as C
from ..ops import _call, _lut_strips, _ptr, _query, _require_gpu, make_shape


def _index32(t):
    """Pixel indices of any integer dtype as contiguous int32 (uint16, as the DSEC h5 files hold them, through its bit pattern:
    torch's unsigned 16-bit type has few kernels of its own)."""
    if t.dtype == torch.uint16:
        t = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return _c(t, torch.int32)


def ingest_events(x, y, t_us, p, counts, image_shape, num_bins, want_voxel_input=False, order_for=None, rectify_map=None):
    """x, y, p: [B, N] float32; t_us: [B, N] int64 (increasing per sample); counts: [B] valid lengths.
    Returns {'events': [B, M, 6], 'num_pos_events': int, 'xytp': [B, N, 4] or None}.
    One host round trip (two integers) sizes the output, as the reference's CPU collate does.
    order_for: a FocusLoss -- the rows of each polarity block are then ordered by (time bin, LUT strip) for that loss
    (FocusLoss.order_events) and the dict carries 'event_offsets'; `calc` gives the same loss and gradient bit for bit.
    rectify_map: [Hs, Ws, 2] float32, contiguous, on the device -- the DSEC `rectify_ev_map`, last axis (x_rect, y_rect) as
    `rectify_events(...).T` unpacks it (loader.py:153,187-189).  x and y are then the raw sensor pixel INDICES (int32 is read
    as it is, other integer dtypes are converted with torch first, floating tensors raise TypeError) and every kernel gathers
    rectify_map[y, x] in its coordinate load: no [B, N] float arrays in between.  Everything else is what the call without a map
    computes on the gathered values; 'xytp' carries the rectified coordinates of all rows (loader.py:169).  Hs, Ws need not equal
    image_shape.  UNPINNED: a raw index outside the map (x >= Ws, y >= Hs, negative) raises or wraps in the reference; here the
    row is dropped from 'events' and written to 'xytp' as (-2, -2, t, p), so both taps of the voxel builder fall outside any grid."""
    _require_gpu(x, 'x')
    dev = x.device
    B, N = x.shape
    rect = ()
    if rectify_map is not None:
        if x.is_floating_point() or y.is_floating_point() or x.dtype == torch.bool or y.dtype == torch.bool:
            raise TypeError(f'with rectify_map, x and y are sensor pixel indices of an integer dtype (got {x.dtype}, {y.dtype})')
        _require_gpu(rectify_map, 'rectify_map')
        if rectify_map.ndim != 3 or rectify_map.shape[2] != 2 or rectify_map.dtype != torch.float32 or not rectify_map.is_contiguous():
            raise ValueError(f'rectify_map must be a contiguous float32 [Hs, Ws, 2] tensor (got {tuple(rectify_map.shape)}, {rectify_map.dtype})')
        x = _index32(x); y = _index32(y); p = p.float().contiguous()
        rect = (int(rectify_map.shape[0]), int(rectify_map.shape[1]), _ptr(rectify_map))
    else:
        x = x.float().contiguous(); y = y.float().contiguous(); p = p.float().contiguous()
    sym = 'mpc_ingest_rect_' if rect else 'mpc_ingest_'
    t_us = t_us.to(torch.int64).contiguous()
    cnt = counts.to(device=dev, dtype=torch.int32).contiguous()
    shape = C.IngestShape(B=B, N=N, H=int(image_shape[0]), W=int(image_shape[1]), nb=int(num_bins))
    ws = torch.empty(max(_query('mpc_ingest_workspace_bytes', dev, ctypes.byref(shape)), 256), dtype=torch.uint8, device=dev)
    out_max = torch.empty(2, dtype=torch.int32, device=dev)
    _call(sym + 'count', dev, ctypes.byref(shape), *rect, _ptr(x), _ptr(y), _ptr(t_us), _ptr(p), _ptr(cnt), _ptr(out_max), _ptr(ws))
    max_pos, max_neg = (int(v) for v in out_max.tolist())          # the collate's host decision
    events = torch.empty((B, max_pos + max_neg, 6), dtype=torch.float32, device=dev)
    xytp = torch.empty((B, N, 4), dtype=torch.float32, device=dev) if want_voxel_input else None
    if order_for is not None:
        # the rows are written in bucket order right away (mpc_ingest_scatter_ordered): no ordering pass over the tensor
        cfg = order_for._cfg
        lshape = make_shape(cfg, B, max_pos + max_neg, max_pos if cfg.polarity_split else max_pos + max_neg, 1)
        ncs = _lut_strips(lshape, dev)
        if ncs > 0 and cfg.polarity_split and tuple(cfg.image_shape) == (int(image_shape[0]), int(image_shape[1])) and cfg.num_bins == int(num_bins):
            nb2 = _query('mpc_ingest_ordered_workspace_bytes', dev, ctypes.byref(shape), ctypes.byref(lshape))
            ws2 = torch.empty(max(nb2, 256), dtype=torch.uint8, device=dev)
            offs = torch.empty((B, 2, cfg.num_bins * ncs + 1), dtype=torch.int32, device=dev)
            _call(sym + 'scatter_ordered', dev, ctypes.byref(shape), ctypes.byref(lshape), *rect, _ptr(x), _ptr(y), _ptr(t_us), _ptr(p),
                  _ptr(cnt), max_pos, max_neg, _ptr(events), _ptr(offs), _ptr(xytp), _ptr(ws), _ptr(ws2))
            return {'events': events, 'num_pos_events': max_pos, 'xytp': xytp, 'event_offsets': offs}
    _call(sym + 'scatter', dev, ctypes.byref(shape), *rect, _ptr(x), _ptr(y), _ptr(t_us), _ptr(p), _ptr(cnt),
          max_pos, max_neg, _ptr(events), _ptr(xytp), _ptr(ws))
    out = {'events': events, 'num_pos_events': max_pos, 'xytp': xytp}
    return out if order_for is None else order_for.order_events(out)


_EDGES = {}          # (device, num_bins) -> the fp32 bin edges of the EVIMO2 loader on that device


def _window_edges(dev, num_bins):
    """torch.linspace(0, 1, num_bins + 1) as the CPU computes it (datasubset.py:77), uploaded once per (device, num_bins)."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), int(num_bins))
    e = _EDGES.get(key)
    if e is None:
        e = _EDGES[key] = torch.linspace(0, 1, int(num_bins) + 1, dtype=torch.float32, device='cpu').to(dev)
    return e


def _c(t, dtype=None):
    t = t if dtype is None or t.dtype == dtype else t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


def ingest_raw_events(x, y, t_us, p, counts, num_bins, dataset, *, flow_duration_ms=None, polarity_aware_batching=True,
                      xy_scale=None, order_for=None):
    """The loss events of the EVIMO2 / MultiFlow configurations from the padded raw window `representation_grids` takes.

    x, y, p: [B, N]; t_us: [B, N] int64, NON-DECREASING per sample; counts: [B] valid lengths.  x / y are read as int32 or fp32
    and p as fp32 or int64 without a conversion pass; other dtypes are converted with torch on the device first.  p is in
    {0, 1}; for EVIMO2 it is the flipped polarity `1 - p` of datasubset.py:154.
    dataset='evimo2' (flow_duration_ms required): datasubset.py:206-215.  The reference cuts the window, normalises time and
        bins in FLOAT32 (`ts[-1] - flow_duration * 1e3` promotes to fp32, where one ulp of a microsecond stamp is 4 to 16 us);
        the kernels restate that chain operation by operation, with the bin edges of torch.linspace as the CPU computes them
        (cached on the device per (device, num_bins)).  Events with fp32(t) <= fp32(t_last) - fp32(flow_duration_ms * 1e3) are
        dropped.  A sample with counts[b] == 0 gives zero rows (the reference raises on `ts[-1]`).
    dataset='multiflow' (flow_duration_ms rejected): sample.py:224-236 -- (t - min) / (max - min) in float64 over the
        window's counts[b] events, np.linspace edges, cast to fp32 last; the caller cuts the window (sample.py:156-170).
    Neither has an in-image filter.  polarity_aware_batching=True: rows with p == 1, zero padded to the batch maximum, then
    rows with p == 0 (data_loading.py:38-43), `num_pos_events` = the positive maximum; False: one block per sample in input
    order and `num_pos_events` = -1, as the reference's collate returns.
    xy_scale=(x_scale, y_scale): column 0 is y * fp32(y_scale) and column 1 x * fp32(x_scale), one fp32 multiply each when the
        row is written (EVIMO2's X_SCALE / Y_SCALE = 0.8).  UNPINNED: the reference hands the two scales along
        (datasubset.py:227-228) but ships no code that applies them.  None leaves the coordinates as they are.
    order_for: a FocusLoss -- the result goes through its `order_events` (a second pass over the tensor) and carries
        'event_offsets'.
    Returns {'events': [B, M, 6] float32, 'num_pos_events': int}.  One host round trip (two integers) sizes the output."""
    if dataset not in ('evimo2', 'multiflow'):
        raise ValueError(f"dataset must be 'evimo2' or 'multiflow', got {dataset!r}")
    if dataset == 'evimo2':
        if flow_duration_ms is None:
            raise ValueError("dataset='evimo2' needs flow_duration_ms (EVIMO2_Datasubset's flow_time)")
        if not float(flow_duration_ms) >= 0:
            raise ValueError(f'flow_duration_ms must not be negative, got {flow_duration_ms}')
    elif flow_duration_ms is not None:
        raise ValueError("dataset='multiflow' takes no flow_duration_ms: the caller cuts the window (sample.py:156-170)")
    for name, t in (('x', x), ('y', y), ('t_us', t_us), ('p', p)):
        _require_gpu(t, name)
    if not (x.shape == y.shape == p.shape == t_us.shape) or x.ndim != 2:
        raise ValueError(f'x, y, t_us, p must share one [B, N] shape (got {tuple(x.shape)}, {tuple(y.shape)}, '
                         f'{tuple(t_us.shape)}, {tuple(p.shape)})')
    dev = x.device
    B, N = x.shape
    if counts.ndim != 1 or counts.shape[0] != B:
        raise ValueError(f'counts must be [B] = [{B}], got {tuple(counts.shape)}')
    xy_int = x.dtype == torch.int32 and y.dtype == torch.int32
    if xy_int:
        x, y = _c(x), _c(y)
    else:
        x, y = _c(x, torch.float32), _c(y, torch.float32)
    p_int64 = p.dtype == torch.int64
    p = _c(p) if p_int64 else _c(p, torch.float32)
    t_us = _c(t_us, torch.int64)
    cnt = _c(counts.to(dev), torch.int32)
    xs, ys = (1.0, 1.0) if xy_scale is None else (float(xy_scale[0]), float(xy_scale[1]))
    evimo2 = dataset == 'evimo2'
    shape = C.WindowShape(B=B, N=N, nb=int(num_bins), time_mode=C.WINDOW_TIME_FP32_SUFFIX if evimo2 else C.WINDOW_TIME_MINMAX64,
                          xy_int=int(xy_int), p_int64=int(p_int64), split=int(bool(polarity_aware_batching)),
                          duration_us=float(flow_duration_ms) * 1e3 if evimo2 else 0.0, x_scale=xs, y_scale=ys)
    nbytes = _query('mpc_ingest_window_workspace_bytes', dev, ctypes.byref(shape))
    edges = _window_edges(dev, num_bins) if evimo2 else None
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    out_max = torch.empty(2, dtype=torch.int32, device=dev)
    _call('mpc_ingest_window_count', dev, ctypes.byref(shape), _ptr(t_us), _ptr(p), _ptr(cnt), _ptr(out_max), _ptr(ws))
    max_pos, max_neg = (int(v) for v in out_max.tolist())          # the collate's host decision
    events = torch.empty((B, max_pos + max_neg, 6), dtype=torch.float32, device=dev)
    _call('mpc_ingest_window_scatter', dev, ctypes.byref(shape), _ptr(x), _ptr(y), _ptr(t_us), _ptr(p), _ptr(cnt), _ptr(edges),
          max_pos, max_neg, _ptr(events), _ptr(ws))
    out = {'events': events, 'num_pos_events': max_pos if polarity_aware_batching else -1}
    return out if order_for is None else order_for.order_events(out)
