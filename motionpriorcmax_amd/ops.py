"""torch-facing wrappers of the HIP kernels behind include/mpcmax.h.

PyTorch is used only for device memory, the current HIP stream and autograd plumbing; every
numerical step of the path runs in libmpcmax.so.  Tensors must live on a GPU: there is no CPU
or eager fallback (a CPU tensor raises)."""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import torch

from . import _lib as C


@dataclass(frozen=True)
class PathConfig:
    """Static configuration of one FocusLoss instance (reference focus.py:28-45)."""
    image_shape: tuple
    num_tref: int
    num_bins: int
    num_knn: int
    smooth_weight: float
    sp: int
    norm_l2: bool
    dist_l1: bool
    scale_by_dt: bool
    mask_border: bool
    polarity_split: bool
    scheme_iwd: bool
    smooth_on_next: bool
    variance: bool = False
    atomic_path: bool = False
    pyramid_levels: int = 1       # UNPINNED extension: levels of the IWE pyramid every route serves (iwe_pyramid_pass); 1 = the reference

    def flags(self):
        f = 0
        f |= C.F_SCALE_BY_DT if self.scale_by_dt else 0
        f |= C.F_MASK_BORDER if self.mask_border else 0
        f |= C.F_POLARITY_SPLIT if self.polarity_split else 0
        f |= C.F_NORM_L2 if self.norm_l2 else 0
        f |= C.F_OBJ_VARIANCE if self.variance else 0
        f |= C.F_DIST_L1 if self.dist_l1 else 0
        f |= C.F_SCHEME_IWD if self.scheme_iwd else 0
        f |= C.F_WANT_NEXT if (self.smooth_on_next and self.smooth_weight > 0) else 0
        f |= C.F_ATOMIC_PATH if self.atomic_path else 0
        return f

    @property
    def lut_grid(self):
        h, w = self.image_shape
        return (h + self.sp - 1) // self.sp, (w + self.sp - 1) // self.sp


class StageTimer:
    """Optional per-stage HIP-event timing (bench.py): events are recorded on the stream the
    kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = {}

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = {'launches': len(ms), 'avg_us': 1e3 * sum(ms) / max(len(ms), 1)}
        return out


STAGE_TIMER = None   # set to a StageTimer to time every C-ABI call


_KERNEL_TIMERS = [0]


def kernel_timer_on():
    """True inside `with KernelTimer()`: the library brackets every launch with HIP events then, which must not fall into a graph
    capture -- and a replayed graph would show the timer nothing."""
    return _KERNEL_TIMERS[0] > 0


class KernelTimer:
    """Per-KERNEL HIP-event timing by the library itself (mpc_profile_start / mpc_profile_stop: two events around every
    launch, on the launch stream).  `with KernelTimer() as kt: ...steps...` then kt.summary() ->
    {kernel name: {'launches': n, 'avg_us': mean duration of a launch, 'total_us': sum}}.  Diagnostics (bench.py)."""

    def __enter__(self):
        C.lib().mpc_profile_start()
        _KERNEL_TIMERS[0] += 1
        self.records = None
        return self

    def __exit__(self, *exc):
        _KERNEL_TIMERS[0] -= 1
        torch.cuda.synchronize()
        cap = 1 << 16
        names = ctypes.create_string_buffer(cap * 48)
        ms = (ctypes.c_float * cap)()
        n = int(C.lib().mpc_profile_stop(names, len(names), ms, cap))
        out = {}
        for nm, t in zip(names.value.decode().split('\n')[:n], ms[:n]):
            k = nm.strip().lstrip('(').split('<')[0].rstrip(')').strip()
            r = out.setdefault(k, {'launches': 0, 'total_us': 0.0})
            r['launches'] += 1
            r['total_us'] += 1e3 * t
        for r in out.values():
            r['avg_us'] = r['total_us'] / r['launches']
        self.records = out
        return False

    def summary(self):
        return self.records or {}


def _is_current(device):
    # the library launches on the CURRENT HIP device: the tensors' device has to be current for the call (tensors on
    # cuda:1 while cuda:0 is current would otherwise launch in the wrong device context).  The usual case -- it is
    # current already -- skips the guard object (~10 us of host time per call, a B = 1 step is host bound)
    idx = device.index
    return idx is None or idx == torch.cuda.current_device()


class _stage:
    def __init__(self, name, device):
        self.name, self.device = name, device

    def __enter__(self):
        self.guard = None if _is_current(self.device) else torch.cuda.device(self.device)
        if self.guard is not None:
            self.guard.__enter__()
        if STAGE_TIMER is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.device))

    def __exit__(self, *exc):
        if STAGE_TIMER is not None:
            self.b.record(torch.cuda.current_stream(self.device))
            STAGE_TIMER.records.setdefault(self.name, []).append((self.a, self.b))
        if self.guard is not None:
            self.guard.__exit__(*exc)
        return False


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a GPU tensor: the CMax path runs in libmpcmax.so (HIP, '
                           f'gfx950) and has no CPU fallback (got device {t.device})')


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_DT_CODE = {torch.float32: C.DT_F32, torch.float16: C.DT_F16, torch.bfloat16: C.DT_BF16}


def _net(t: torch.Tensor):
    """A network tensor (the coefficient grid, the convex-upsampling mask) for a `_dt` entry point -> (the tensor's OWN contiguous
    storage where it is fp32, fp16 or bf16 -- no upcast copy: the kernels convert at the load, exactly --, else an fp32 copy; its
    MPC_DT_* code).  The gradient goes back in that dtype, rounded once by the kernel that computes it."""
    t = t.detach()
    if t.dtype not in _DT_CODE:
        t = t.float()
    return t.contiguous(), _DT_CODE[t.dtype]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(device):
    """Handle of torch's CURRENT stream on `device` (the library launches on it)."""
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))        # ~1 us; the Stream object below costs ~15
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _call(name, dev, *args, label=None, accept=()):
    """THE way into a launch symbol of libmpcmax.so: `name`(*args, stream) with `dev` current, on torch's current stream of `dev`,
    timed as stage `label` when a StageTimer is set; a return code other than 0 raises the library's error under `name`, except
    the codes in `accept`, which are handed back (a call that may answer MPC_E_UNSUPPORTED).  The label is an interface --
    bench.py keys its byte counts and its kernel-to-stage map on it -- and is the symbol's name unless `label` says otherwise.
    Pointers are spelt at the call site (_ptr): this function does nothing per argument, and with no timer set and `dev` current
    already it builds no _stage either (a B = 1 step is host bound: ~1 us per call, two calls per fused step)."""
    fn = getattr(C.lib(), name)
    if STAGE_TIMER is None and _is_current(dev):
        rc = fn(*args, _stream(dev))
    else:
        with _stage(label or name, dev):
            rc = fn(*args, _stream(dev))
    if rc != 0 and rc not in accept:
        C.check(rc, name)
    return rc


def _query(name, dev, *args, accept=()):
    """A host-side question to libmpcmax.so (a size, a count, whether a shape is served: no launch, no stream) as an int, asked with
    `dev` current: the workspace layouts follow the CU count of the device the kernels will run on (api.hip: mpc_layout).  A
    negative answer is an error code and raises the library's error, except the codes in `accept`."""
    fn = getattr(C.lib(), name)
    if _is_current(dev):
        n = int(fn(*args))
    else:
        with torch.cuda.device(dev):
            n = int(fn(*args))
    if n < 0 and n not in accept:
        C.check(n, name)
    return n


def make_shape(cfg: PathConfig, B, M, Mp, n, extra_flags=0, K=None):
    hq, wq = cfg.lut_grid
    return C.Shape(B=B, M=M, Mp=Mp, nb=cfg.num_bins, T=cfg.num_tref, H=cfg.image_shape[0],
                   W=cfg.image_shape[1], sp=cfg.sp, hq=hq, wq=wq, n=n,
                   K=cfg.num_knn if K is None else K, flags=cfg.flags() | extra_flags)


def alloc_workspace(shape: C.Shape, device) -> torch.Tensor:
    return torch.empty(max(_query('mpc_workspace_bytes', device, ctypes.byref(shape)), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------
# stage wrappers (no autograd)
# ------------------------------------------------------------------------------------------
def knn_lut_fwd(cfg, shape, traj, ws, want_idx=False, idx_out=None):
    """mpc_knn_lut_fwd; want_idx: also the sorted neighbour lists [B, nb, Q, K] int32, into `idx_out` where the caller has the place."""
    dev = traj.device
    B, nb, T, K = shape.B, shape.nb, shape.T, shape.K
    hq, wq = shape.hq, shape.wq
    Q = hq * wq
    flow_lut = torch.empty((B, nb, hq, wq, T, 2), dtype=torch.float32, device=dev)
    flow_next = None
    if shape.flags & C.F_WANT_NEXT:
        flow_next = torch.empty((B, max(nb - 1, 0), hq, wq, 1, 2), dtype=torch.float32, device=dev)
    state = torch.empty(_query('mpc_knn_state_floats', dev, ctypes.byref(shape)), dtype=torch.float32, device=dev)
    idx = (idx_out if idx_out is not None else torch.empty((B, nb, Q, K), dtype=torch.int32, device=dev)) if want_idx else None
    _call('mpc_knn_lut_fwd', dev, ctypes.byref(shape), _ptr(traj), _ptr(flow_lut), _ptr(flow_next), _ptr(state), _ptr(idx), _ptr(ws))
    return flow_lut, flow_next, state, idx


def knn_lut_bwd(shape, traj, g_lut, g_next, state, ws):
    g_traj = torch.empty_like(traj)
    _call('mpc_knn_lut_bwd', traj.device, ctypes.byref(shape), _ptr(traj), _ptr(g_lut), _ptr(g_next), _ptr(state), _ptr(g_traj), _ptr(ws))
    return g_traj


# ------------------------------------------------------------------------------------------
# more trajectories per sample than the 16-bit tables of mpc_knn_lut_fwd hold (n >= 65536): csrc/knn_wide.hip
# ------------------------------------------------------------------------------------------
KNN_CHUNK = 65535     # points per search of the chunked route, at most 65535 (what mpc_knn_lut_fwd serves); tests lower it
KNN_MAX_CHUNKS = 64   # csrc/knn_wide.hip: one lane per chunk of a query


def knn_is_wide(n):
    """Does a point set of n trajectories per sample take the chunked route (knn_wide_fwd)?  n >= 65536 with the shipped KNN_CHUNK."""
    return n > KNN_CHUNK


def _wide_limit(what, n):
    return ValueError(f'{what} serves at most {KNN_CHUNK} trajectories per sample, got {n}: larger point sets run the chunked '
                      f'neighbour search (ops.knn_wide_fwd), which has no captured or pyramid form')


def knn_chunk_starts(n, K):
    """The chunked route's contiguous index ranges: ceil(n / KNN_CHUNK) chunks of near-equal length, as C + 1 starts."""
    if not 1 <= KNN_CHUNK <= 65535:
        raise ValueError(f'KNN_CHUNK={KNN_CHUNK} outside [1, 65535]')
    nc = -(-n // KNN_CHUNK)
    base, rem = divmod(n, nc)
    if nc > KNN_MAX_CHUNKS or base < K:
        raise ValueError(f'n={n} in chunks of {KNN_CHUNK}: {nc} chunks of {base} points; at most {KNN_MAX_CHUNKS} chunks of at least '
                         f'num_knn={K} points are served')
    starts = [0]
    for c in range(nc):
        starts.append(starts[-1] + base + (1 if c < rem else 0))
    return starts


def knn_wide_fwd(cfg, shape, traj):
    """The KNN LUT of n >= 65536 points: the exact search of mpc_knn_lut_fwd on every contiguous index chunk (its sorted neighbour
    lists kept, its LUT dropped), then mpc_knn_merge_fwd: the K smallest of the union by (distance, index) and the interpolation.
    Slicing and copies are torch's, the numerics the library's.  -> (flow_lut, flow_next or None, merged indices [B, nb, Q, K])."""
    dev = traj.device
    B, nb, T, K, n = shape.B, shape.nb, shape.T, shape.K, shape.n
    hq, wq = shape.hq, shape.wq
    Q = hq * wq
    starts = knn_chunk_starts(n, K)
    nc = len(starts) - 1
    cand = torch.empty((nc, B, nb, Q, K), dtype=torch.int32, device=dev)
    ws, ws_len = None, -1
    for c in range(nc):
        lo, hi = starts[c], starts[c + 1]
        # (the search looks at the mid-time rows only: one reference row goes along for the layout, the LUT it gives is dropped)
        sub = traj[:, T - 1:, lo:hi].contiguous()
        cs = C.Shape(B=B, M=0, Mp=0, nb=nb, T=1, H=shape.H, W=shape.W, sp=shape.sp, hq=hq, wq=wq, n=hi - lo, K=K, flags=shape.flags & C.F_DIST_L1)
        if hi - lo != ws_len:
            ws, ws_len = alloc_workspace(cs, dev), hi - lo
        knn_lut_fwd(cfg, cs, sub, ws, want_idx=True, idx_out=cand[c])
    flow_lut = torch.empty((B, nb, hq, wq, T, 2), dtype=torch.float32, device=dev)
    flow_next = None
    if shape.flags & C.F_WANT_NEXT:
        flow_next = torch.empty((B, max(nb - 1, 0), hq, wq, 1, 2), dtype=torch.float32, device=dev)
    idx = torch.empty((B, nb, Q, K), dtype=torch.int32, device=dev)
    _call('mpc_knn_merge_fwd', dev, ctypes.byref(shape), _ptr(traj), _ptr(cand), (ctypes.c_int32 * (nc + 1))(*starts), nc, _ptr(idx),
          _ptr(flow_lut), _ptr(flow_next))
    return flow_lut, flow_next, idx


def knn_idx_bwd(shape, traj, g_lut, g_next, idx):
    """mpc_knn_idx_bwd: dL/dtrajectories from dL/dLUT (and dL/dflow_next) over the merged index lists of knn_wide_fwd."""
    dev = traj.device
    g_traj = torch.empty_like(traj)
    ws = torch.empty(max(_query('mpc_knn_wide_workspace_bytes', dev, ctypes.byref(shape)), 256), dtype=torch.uint8, device=dev)
    _call('mpc_knn_idx_bwd', dev, ctypes.byref(shape), _ptr(traj), _ptr(idx), _ptr(g_lut), _ptr(g_next), _ptr(g_traj), _ptr(ws))
    return g_traj


def event_splat_fwd(shape, events, flow_lut, t_ref, ws):
    dev = events.device
    P = 2 if shape.flags & C.F_POLARITY_SPLIT else 1
    raw = torch.empty((shape.B * shape.T, P, shape.H, shape.W), dtype=torch.float32, device=dev)
    _call('mpc_event_splat_fwd', dev, ctypes.byref(shape), _ptr(events), _ptr(flow_lut), _ptr(t_ref), _ptr(raw), _ptr(ws))
    return raw


def event_splat_fwd_fixed(shape, events, flow_lut, t_ref, ws):
    """mpc_event_splat_fwd_fixed: the raw IWE of these event rows as Q33.30 accumulators (int64), for an exact sum over shards."""
    dev = events.device
    P = 2 if shape.flags & C.F_POLARITY_SPLIT else 1
    fixed = torch.empty((shape.B * shape.T, P, shape.H, shape.W), dtype=torch.int64, device=dev)
    _call('mpc_event_splat_fwd_fixed', dev, ctypes.byref(shape), _ptr(events), _ptr(flow_lut), _ptr(t_ref), _ptr(fixed), _ptr(ws))
    return fixed


def iwe_from_fixed(fixed):
    raw = torch.empty(fixed.shape, dtype=torch.float32, device=fixed.device)
    _call('mpc_iwe_from_fixed', fixed.device, _ptr(fixed), _ptr(raw), fixed.numel())
    return raw


def contrast_fwd(shape, raw, ws, want_grad):
    blur = torch.empty_like(raw)
    gimg = torch.empty_like(raw) if want_grad else None
    _call('mpc_contrast_fwd', raw.device, ctypes.byref(shape), _ptr(raw), _ptr(blur), _ptr(gimg), _ptr(ws))
    return blur, gimg


def lut_smooth(shape, field, nimg, Cch, weight, ws, want_grad):
    g = torch.empty_like(field) if want_grad else None
    _call('mpc_lut_smooth', field.device, ctypes.byref(shape), _ptr(field), nimg, Cch, float(weight), _ptr(g), _ptr(ws))
    return g


def finalize(shape, smooth_nimg, smooth_C, weight, ws, device):
    scal = torch.empty(C.SCAL_COUNT, dtype=torch.float32, device=device)
    _call('mpc_finalize', device, ctypes.byref(shape), smooth_nimg, smooth_C, float(weight), _ptr(scal), _ptr(ws))
    return scal


def event_splat_bwd(shape, events, flow_lut, t_ref, gimg, scal, grad_out, g_lut, add_term, ws, offs=None):
    # (the ordered entry point serves both layouts -- offs None: the records of the forward; it keeps the stage name bench.py knows)
    _call('mpc_event_splat_bwd_ordered', events.device, ctypes.byref(shape), _ptr(events), _ptr(offs), _ptr(flow_lut), _ptr(t_ref),
          _ptr(gimg), _ptr(scal), _ptr(grad_out), _ptr(g_lut), _ptr(add_term), _ptr(ws), label='mpc_event_splat_bwd')
    return g_lut


def scale(x, a):
    y = torch.empty_like(x)
    _call('mpc_scale', x.device, _ptr(x), _ptr(a), _ptr(y), x.numel())
    return y


# ------------------------------------------------------------------------------------------
# the IWE pyramid as one pass behind any forward (csrc/iwe_pyramid.hip)
# ------------------------------------------------------------------------------------------
def _pyramid_limit(levels, what):
    return ValueError(f'pyramid_levels={levels}: {what} (the IWE pyramid serves 2 .. 6 levels of the gradient-magnitude objective at '
                      f'num_tref == 1, on images divisible by 2^(levels - 1) whose coarsest level is at least 3x3)')


def iwe_pyramid_check(cfg: PathConfig, shape, dev):
    """Raises the ValueError of a configuration the pyramid pass does not serve -- BEFORE the route launches anything; the rule
    is the library's (mpc_iwe_pyramid_supported, host only).  Nothing to check at pyramid_levels == 1."""
    if cfg.pyramid_levels > 1:
        rc = _query('mpc_iwe_pyramid_supported', dev, ctypes.byref(shape), cfg.pyramid_levels, accept=(C.E_SHAPE, C.E_UNSUPPORTED))
        if rc:
            raise _pyramid_limit(cfg.pyramid_levels, C.lib().mpc_last_error_string().decode(errors='replace'))


def iwe_pyramid_level_offsets(shape, levels):
    """Float offsets of the unscaled adjoint images of levels 1 .. levels - 1 inside the pass's workspace (include/mpcmax.h:
    the layout is part of the ABI) and their shapes [nimg, H >> l, W >> l]."""
    nimg = shape.B * shape.T * (2 if shape.flags & C.F_POLARITY_SPLIT else 1)
    out, off = [], 0
    for l in range(1, levels):
        h, w = shape.H >> l, shape.W >> l
        out.append((off, (nimg, h, w)))
        off += (nimg * h * w + 63) // 64 * 64
    return out


def iwe_pyramid_pass(shape, levels, raw, gimg, scal, scal_out=None, pws=None, level_scal=None):
    """mpc_iwe_pyramid_fwd behind a forward that left the raw IWE `raw`, the unscaled adjoint image `gimg` (None: no gradient) and
    `scal`: the coarse levels' focus terms go into scal (and scal_out) and their adjoint images into gimg, IN PLACE, in units of
    level 0's coefficient -- the route's backward then runs as it is.  raw / gimg / scal: tensors, or device addresses (int) of
    buffers inside a plan.  `pws`, `level_scal`: the caller's buffers (a captured plan), else allocated here.
    -> (level_scal [levels, SCAL_COUNT], pws)."""
    def addr(t):
        return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    dev = (pws if pws is not None else raw).device
    want_grad = gimg is not None
    if pws is None:
        pws = torch.empty(max(_query('mpc_iwe_pyramid_workspace_bytes', dev, ctypes.byref(shape), levels, int(want_grad)), 256), dtype=torch.uint8, device=dev)
    if level_scal is None:
        level_scal = torch.empty((levels, C.SCAL_COUNT), dtype=torch.float32, device=dev)
    _call('mpc_iwe_pyramid_fwd', dev, ctypes.byref(shape), levels, addr(raw), addr(gimg), addr(scal), addr(scal_out), _ptr(level_scal), _ptr(pws))
    return level_scal, pws


FUSED_CALLS = True    # FocusCalcFn: mpc_focus_fwd / mpc_focus_bwd (two C-ABI calls per step) instead of one call per stage


def _vp(t):
    return None if t is None else t.data_ptr()


class _Plan:
    """What one (configuration, shape) needs on the host and does not change from step to step: the shape struct, the
    workspace size and the layout of ONE float buffer that holds everything the forward leaves for the backward (LUT,
    flow_next, KNN state, smoothness gradient, raw IWE, adjoint image, scalars).  A B = 1 step is host bound: building these
    per step (two ctypes size queries, ~10 torch.empty, two struct fills) cost ~100 us of Python per direction."""

    def __init__(self, cfg, B, M, Mp, n, need_grad, has_offs, dev):
        self.cfg = cfg
        # (bucket-ordered events: the backward reads the rows themselves -- no record region in the workspace either)
        self.shape = make_shape(cfg, B, M, Mp, n, extra_flags=0 if (need_grad and not has_offs) else C.F_NO_BWD_RECORDS)
        self.shape_ref = ctypes.byref(self.shape)
        self.need_grad = need_grad
        iwe_pyramid_check(cfg, self.shape, dev)          # (a plan is built before the first launch of its shape)
        self.ws_bytes = max(_query('mpc_workspace_bytes', dev, self.shape_ref), 256)
        self.pyr_bytes = 0
        if cfg.pyramid_levels > 1:
            self.pyr_bytes = max(_query('mpc_iwe_pyramid_workspace_bytes', dev, self.shape_ref, cfg.pyramid_levels, int(need_grad)), 256)
        s = self.shape
        self.P = 2 if s.flags & C.F_POLARITY_SPLIT else 1
        self.lut_shape = (B, s.nb, s.hq, s.wq, s.T, 2)
        n_lut = B * s.nb * s.hq * s.wq * s.T * 2
        n_nxt = B * max(s.nb - 1, 0) * s.hq * s.wq * 2 if s.flags & C.F_WANT_NEXT else 0
        n_state = _query('mpc_knn_state_floats', dev, self.shape_ref)
        n_gf = 0
        if cfg.smooth_weight > 0 and need_grad:
            n_gf = n_nxt if cfg.smooth_on_next else n_lut
        n_img = B * s.T * self.P * s.H * s.W
        self.img_shape = (B * s.T, self.P, s.H, s.W)
        off = 0
        self.o = {}
        for name, cnt in (('lut', n_lut), ('nxt', n_nxt), ('state', n_state), ('gf', n_gf), ('raw', n_img),
                          ('gimg', n_img if need_grad else 0), ('scal', C.SCAL_COUNT)):
            self.o[name] = (off, cnt)
            off += (cnt + 63) // 64 * 64          # 256-byte aligned pieces
        self.buf_floats = max(off, 64)
        # backward scratch: dL/dLUT and (smoothness on flow_to_next) the scaled dL/dflow_next
        self.n_glut = n_lut
        self.n_gnext = n_gf if (cfg.smooth_on_next and n_gf) else 0
        self.smooth_weight = float(cfg.smooth_weight)

    def io(self, base, traj, ev, tr, blur, offs, scal_out=None):
        def at(name):
            off, cnt = self.o[name]
            return base + 4 * off if cnt else None
        return C.FocusBuffers(traj=traj, events=ev, t_ref=tr, flow_lut=at('lut'), flow_next=at('nxt'), knn_state=at('state'),
                              smooth_grad=at('gf'), iwe_raw=at('raw'), iwe_blur=blur, grad_iwe=at('gimg'), scal=at('scal'),
                              smooth_weight=self.smooth_weight, event_offsets=offs, scal_out=scal_out)

    def view(self, buf, name):
        off, cnt = self.o[name]
        return buf[off:off + cnt] if cnt else None

    def pyramid(self, dev, buf, out3, pws, level_scal):
        """The pyramid pass behind mpc_focus_fwd on this plan's buffer `buf` (pyramid_levels > 1): same stream, plain launches."""
        def at(name):
            off, cnt = self.o[name]
            return buf.data_ptr() + 4 * off if cnt else None
        iwe_pyramid_pass(self.shape, self.cfg.pyramid_levels, at('raw'), at('gimg'), at('scal'), _vp(out3), pws, level_scal)


_PLANS = {}


def _plan(cfg, B, M, Mp, n, need_grad, has_offs, dev):
    # (per device: the workspace layout follows the CU count of the device the step runs on, api.hip: mpc_layout)
    key = (cfg, B, M, Mp, n, need_grad, has_offs, dev.index)
    p = _PLANS.get(key)
    if p is None:
        if len(_PLANS) > 256:
            _PLANS.clear()
        p = _PLANS[key] = _Plan(cfg, B, M, Mp, n, need_grad, has_offs, dev)
    return p


def _focus_fwd_call(p, dev, traj, ev, tr, buf, blur, ws, offs, out3=None):
    io = p.io(buf.data_ptr(), traj.data_ptr(), ev.data_ptr(), tr.data_ptr(), blur.data_ptr(), _vp(offs), _vp(out3))
    _call('mpc_focus_fwd', dev, p.shape_ref, ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()))


def _focus_bwd_call(p, dev, traj, ev, tr, buf, ws, offs, grad_out, scratch, g_traj):
    io = p.io(buf.data_ptr(), traj.data_ptr(), ev.data_ptr(), tr.data_ptr(), None, _vp(offs))
    io.flow_next = None
    io.iwe_raw = None
    g_lut = scratch.data_ptr()
    g_next = g_lut + 4 * ((p.n_glut + 63) // 64 * 64) if p.n_gnext else None
    _call('mpc_focus_bwd', dev, p.shape_ref, ctypes.byref(io), ctypes.c_void_p(grad_out.data_ptr()), ctypes.c_void_p(g_lut),
          ctypes.c_void_p(g_next) if g_next else None, ctypes.c_void_p(g_traj.data_ptr()), ctypes.c_void_p(ws.data_ptr()))


def _bwd_scratch_floats(p):
    return (p.n_glut + 63) // 64 * 64 + p.n_gnext + 64


def event_bucket_order(cfg: PathConfig, events, num_pos):
    """SURVEY.md 8f-1, layout half (mpc_event_bucket_order): the rows of each polarity block of `events` [B, M, 6]
    ordered by (time bin, LUT strip), and the offsets table [B, 2, nb * strips + 1] int32.  The ordered tensor gives
    the same loss and gradient bit for bit; handed to FocusCalcFn together with the table, the step skips one 16-byte
    record per event in each direction.  Done once per batch, outside the training step (it belongs to ingest)."""
    B, M, Mp = _check_events(events, cfg, num_pos)
    dev = events.device
    ev = _f32c(events.detach())
    shape = make_shape(cfg, B, M, Mp, 1)
    ncs = _lut_strips(shape, dev)
    if ncs <= 0:
        raise ValueError('no bucketed event layout for this configuration (num_tref > 1 or the atomic debugging path)')
    out = torch.empty_like(ev)
    offs = torch.empty((B, 2, cfg.num_bins * ncs + 1), dtype=torch.int32, device=dev)
    ws = torch.empty(max(_query('mpc_event_order_workspace_bytes', dev, ctypes.byref(shape)), 256), dtype=torch.uint8, device=dev)
    _call('mpc_event_bucket_order', dev, ctypes.byref(shape), _ptr(ev), _ptr(out), _ptr(offs), _ptr(ws))
    return out, offs


_NCS_CACHE = {}


def _lut_strips(shape, device):
    """LUT strips of the backward buckets for `shape` on `device` (the count follows the device's layout, so the query runs
    under that device and the cache is keyed on it); <= 0: no bucketed layout (a shape the library rejects included)."""
    key = (shape.B, shape.M, shape.Mp, shape.nb, shape.T, shape.H, shape.W, shape.sp, shape.flags, device.index)
    ncs = _NCS_CACHE.get(key)
    if ncs is None:
        ncs = _NCS_CACHE[key] = _query('mpc_event_lut_strips', device, ctypes.byref(shape), accept=(C.E_SHAPE,))
    return ncs


def _check_offsets(offs, cfg, shape, device):
    if offs is None:
        return None
    _require_gpu(offs, "batch['event_offsets']")
    ncs = _lut_strips(shape, device)
    want = (shape.B, 2, cfg.num_bins * ncs + 1)
    if ncs <= 0 or offs.dtype != torch.int32 or tuple(offs.shape) != want or offs.device != device:
        raise ValueError(f"event_offsets must be int32 {want} on {device} (from event_bucket_order with this configuration), "
                         f"got {offs.dtype} {tuple(offs.shape)} on {offs.device}")
    return offs.contiguous()


def _check_events(events, cfg, num_pos):
    _require_gpu(events, "batch['events']")
    if events.dim() != 3 or events.shape[-1] != 6:
        raise ValueError(f"events must be [B, M, 6], got {tuple(events.shape)}")
    B, M, _ = events.shape
    if cfg.polarity_split:
        if not (0 <= num_pos <= M):
            raise ValueError(f'num_pos_events={num_pos} outside [0, {M}]')
        Mp = int(num_pos)
    else:
        Mp = M
    return B, M, Mp


# ------------------------------------------------------------------------------------------
# autograd: the whole loss  trajectories -> (loss, focus, smooth, iwes)
# ------------------------------------------------------------------------------------------
def _calc_inputs(trajectories, events, t_ref, cfg, num_pos):
    _require_gpu(trajectories, 'trajectories')
    B, M, Mp = _check_events(events, cfg, num_pos)
    T, nb = cfg.num_tref, cfg.num_bins
    if trajectories.dim() != 4 or trajectories.shape[0] != B or trajectories.shape[1] != T + nb \
            or trajectories.shape[3] != 2:
        raise ValueError(f'trajectories must be [B={B}, {T + nb}, n, 2], got {tuple(trajectories.shape)}')
    dev = trajectories.device
    traj = _f32c(trajectories.detach())
    ev = _f32c(events.detach())
    tr = _f32c(t_ref.detach().to(dev))
    return B, M, Mp, traj.shape[2], dev, traj, ev, tr


def _staged_fwd(cfg, shape, fshape, traj, ev, tr, ws, need_grad, kshape=None):
    """The loss one library call per stage: KNN LUT -> smoothness (where weighted) -> warp + vote (on `fshape`: `shape`, or without
    backward records for bucket-ordered events) -> blur + objective -> scalars.  The route the tests hold the fused call against
    and bench.py's instrumented pass times; the pyramid starts from it.  `kshape`: the chunked neighbour search of n >= 65536
    trajectories (knn_wide_fwd) on this shape -- `shape` and `ws` then serve the other stages and carry no points (n = 0), and the
    state for the backward is the merged index lists."""
    B, T, nb = shape.B, cfg.num_tref, cfg.num_bins
    if kshape is not None:
        flow_lut, flow_next, state = knn_wide_fwd(cfg, kshape, traj)
    else:
        flow_lut, flow_next, state, _ = knn_lut_fwd(cfg, shape, traj, ws)
    g_field = None
    s_nimg = s_C = 0
    if cfg.smooth_weight > 0:
        if cfg.smooth_on_next:
            field, s_nimg, s_C = flow_next, B * (nb - 1), 2
        else:
            field, s_nimg, s_C = flow_lut, B * nb, 2 * T
        if s_nimg > 0:
            g_field = lut_smooth(shape, field, s_nimg, s_C, cfg.smooth_weight, ws, need_grad)
    raw = event_splat_fwd(fshape, ev, flow_lut, tr, ws)
    blur, gimg = contrast_fwd(shape, raw, ws, need_grad)
    scal = finalize(shape, s_nimg, s_C, cfg.smooth_weight, ws, traj.device)
    return flow_lut, state, g_field, raw, blur, gimg, scal


def _staged_bwd(cfg, shape, traj, ev, tr, flow_lut, state, gimg, scal, g_field, g, ws, offs=None, kshape=None):
    """The backward of _staged_fwd from the adjoint image to dL/dtrajectories: event backward (+ smoothness) -> KNN backward
    (`kshape`: over the merged index lists, knn_idx_bwd)."""
    g_next = None
    g_lut = torch.empty_like(flow_lut)
    if g_field is not None and not cfg.smooth_on_next:
        event_splat_bwd(shape, ev, flow_lut, tr, gimg, scal, g, g_lut, g_field, ws, offs)   # smoothness folded in
    else:
        event_splat_bwd(shape, ev, flow_lut, tr, gimg, scal, g, g_lut, None, ws, offs)
        if g_field is not None:
            g_next = scale(g_field, g)
    if kshape is not None:
        return knn_idx_bwd(kshape, traj, g_lut, g_next, state)
    return knn_lut_bwd(shape, traj, g_lut, g_next, state, ws)


class FocusCalcFn(torch.autograd.Function):
    """FocusLoss.calc (reference focus.py:66-113) as one differentiable op: KNN LUT -> smoothness
    -> warp + vote -> blur + objective in forward, hand-derived backward to `trajectories`."""

    @staticmethod
    def forward(ctx, trajectories, events, t_ref, cfg: PathConfig, num_pos: int, event_offsets=None):
        B, M, Mp, n, dev, traj, ev, tr = _calc_inputs(trajectories, events, t_ref, cfg, num_pos)
        need_grad = trajectories.requires_grad
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)      # no zero-filled [B,P,H,W] gradient for the detached outputs

        wide = knn_is_wide(n)
        if wide and cfg.pyramid_levels > 1:
            raise _wide_limit('pyramid_levels > 1', n)
        if STAGE_TIMER is None and FUSED_CALLS and not wide:
            # one C-ABI call for the whole forward (mpc_focus_fwd issues the same launches); per-shape host state is cached
            p = _plan(cfg, B, M, Mp, n, need_grad, event_offsets is not None, dev)
            offs = _check_offsets(event_offsets, cfg, p.shape, dev)
            ws = torch.empty(p.ws_bytes, dtype=torch.uint8, device=dev)
            buf = torch.empty(p.buf_floats, dtype=torch.float32, device=dev)
            blur = torch.empty(p.img_shape, dtype=torch.float32, device=dev)
            # (the outputs must not alias the saved scalars: the library writes loss / focus / smooth a second time into `out` --
            # io.scal_out -- instead of the host cloning them with a kernel of its own)
            out = torch.empty(3, dtype=torch.float32, device=dev)
            _focus_fwd_call(p, dev, traj, ev, tr, buf, blur, ws, offs, out)
            if cfg.pyramid_levels > 1:
                # (the pass's workspace lives for the forward only: the backward reads the folded adjoint image)
                p.pyramid(dev, buf, out, torch.empty(p.pyr_bytes, dtype=torch.uint8, device=dev),
                          torch.empty((cfg.pyramid_levels, C.SCAL_COUNT), dtype=torch.float32, device=dev))
            ctx.plan, ctx.ws, ctx.offs = p, ws, offs
            ctx.save_for_backward(traj, ev, tr, buf)
            loss, focus, smooth = out[C.SCAL_LOSS], out[C.SCAL_FOCUS], out[C.SCAL_SMOOTH]
            ctx.mark_non_differentiable(focus, smooth, blur)
            return loss, focus, smooth, blur

        # (n >= 65536: the neighbour search runs in chunks on a shape of its own; the other stages' shape and workspace carry no points)
        kshape = make_shape(cfg, B, 0, 0, n) if wide else None
        ns, Ks = (0, 0) if wide else (n, None)
        shape = make_shape(cfg, B, M, Mp, ns, extra_flags=0 if need_grad else C.F_NO_BWD_RECORDS, K=Ks)
        ws = alloc_workspace(shape, dev)
        offs = _check_offsets(event_offsets, cfg, shape, dev)
        fshape = shape if offs is None else make_shape(cfg, B, M, Mp, ns, extra_flags=C.F_NO_BWD_RECORDS, K=Ks)
        iwe_pyramid_check(cfg, shape, dev)
        flow_lut, state, g_field, raw, blur, gimg, scal = _staged_fwd(cfg, shape, fshape, traj, ev, tr, ws, need_grad, kshape)
        if cfg.pyramid_levels > 1:
            iwe_pyramid_pass(shape, cfg.pyramid_levels, raw, gimg, scal)
        ctx.plan = None
        ctx.shape, ctx.kshape = shape, kshape
        ctx.offs = offs
        ctx.ws = ws
        ctx.save_for_backward(traj, ev, tr, flow_lut, state, gimg, scal, g_field)
        out = scal[:3].clone()                # one tiny copy: the outputs must not alias the saved scalars
        loss, focus, smooth = out[C.SCAL_LOSS], out[C.SCAL_FOCUS], out[C.SCAL_SMOOTH]
        ctx.mark_non_differentiable(focus, smooth, blur)
        return loss, focus, smooth, blur

    @staticmethod
    def backward(ctx, g_loss, g_focus, g_smooth, g_iwes):
        if g_loss is None:
            return None, None, None, None, None, None
        g = _f32c(g_loss.reshape(1))
        cfg, ws, offs = ctx.cfg, ctx.ws, ctx.offs
        if ctx.plan is not None:
            p = ctx.plan
            traj, ev, tr, buf = ctx.saved_tensors
            scratch = torch.empty(_bwd_scratch_floats(p), dtype=torch.float32, device=traj.device)
            g_traj = torch.empty_like(traj)
            _focus_bwd_call(p, traj.device, traj, ev, tr, buf, ws, offs, g, scratch, g_traj)
            return g_traj, None, None, None, None, None
        shape = ctx.shape
        traj, ev, tr, flow_lut, state, gimg, scal, g_field = ctx.saved_tensors
        return _staged_bwd(cfg, shape, traj, ev, tr, flow_lut, state, gimg, scal, g_field, g, ws, offs, ctx.kshape), None, None, None, None, None


class PyramidFocusFn(torch.autograd.Function):
    """UNPINNED EXTENSION, default off (FocusLoss(pyramid_levels=L > 1)): FocusLoss.calc with an IWE pyramid -- BASELINE.json's
    configs[2] names one, the reference has none (focus.py:90-91 evaluates one scale), so this is a definition, not a port:
    level l + 1 is the 2x2 average of the RAW level-l IWE, every level goes through the reference's own blur + gradient-magnitude
    objective (mpc_contrast_fwd on a shape of that level's size), and the focus term is the sum of the levels' 1 / val.
    Stage calls (no fused path); `iwes` are the blurred level-0 images.  FocusLoss(pyramid_fused=False) runs it: the cross-check of
    the fused pass (iwe_pyramid_pass), which serves every route by default."""

    @staticmethod
    def forward(ctx, trajectories, events, t_ref, cfg: PathConfig, num_pos: int, levels: int):
        B, M, Mp, n, dev, traj, ev, tr = _calc_inputs(trajectories, events, t_ref, cfg, num_pos)
        if knn_is_wide(n):
            raise _wide_limit('pyramid_levels > 1', n)
        H, W = cfg.image_shape
        if H % (1 << (levels - 1)) or W % (1 << (levels - 1)) or min(H, W) >> (levels - 1) < 3:
            raise ValueError(f'pyramid_levels={levels}: image shape {H}x{W} must be divisible by {1 << (levels - 1)} and stay >= 3 pixels')
        need_grad = trajectories.requires_grad
        shape = make_shape(cfg, B, M, Mp, n, extra_flags=0 if need_grad else C.F_NO_BWD_RECORDS)
        ws = alloc_workspace(shape, dev)
        flow_lut, state, g_field, raw, blur0, gimg0, scal0 = _staged_fwd(cfg, shape, shape, traj, ev, tr, ws, need_grad)
        nimg = raw.shape[0] * raw.shape[1]
        gimgs, scals, sizes = [gimg0], [scal0], [(H, W)]
        focus_total = scal0[C.SCAL_FOCUS].clone()
        cur, h, w = raw, H, W
        for lv in range(1, levels):
            nxt = torch.empty((raw.shape[0], raw.shape[1], h // 2, w // 2), dtype=torch.float32, device=dev)
            _call('mpc_pool2_fwd', dev, _ptr(cur), _ptr(nxt), nimg, h, w)
            h, w = h // 2, w // 2
            cfg_l = PathConfig(**{**cfg.__dict__, 'image_shape': (h, w), 'smooth_weight': 0.0})
            sh_l = make_shape(cfg_l, B, 0, 0, 0, K=0)
            ws_l = alloc_workspace(sh_l, dev)
            _, g_l = contrast_fwd(sh_l, nxt, ws_l, need_grad)
            sc_l = finalize(sh_l, 0, 0, 0.0, ws_l, dev)
            gimgs.append(g_l); scals.append(sc_l); sizes.append((h, w))
            focus_total = focus_total + sc_l[C.SCAL_FOCUS]
            cur = nxt
        ctx.cfg, ctx.shape, ctx.ws, ctx.nimg, ctx.sizes = cfg, shape, ws, nimg, sizes
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(traj, ev, tr, flow_lut, state, g_field, *scals, *([g for g in gimgs] if need_grad else []))
        ctx.levels = levels
        smooth = scal0[C.SCAL_SMOOTH].clone()
        loss = focus_total + smooth
        ctx.mark_non_differentiable(focus_total, smooth, blur0)
        return loss, focus_total, smooth, blur0

    @staticmethod
    def backward(ctx, g_loss, g_focus, g_smooth, g_iwes):
        if g_loss is None:
            return None, None, None, None, None, None
        cfg, shape, ws, L = ctx.cfg, ctx.shape, ctx.ws, ctx.levels
        saved = ctx.saved_tensors
        traj, ev, tr, flow_lut, state, g_field = saved[:6]
        scals, gimgs = saved[6:6 + L], list(saved[6 + L:6 + 2 * L])
        # (the coarser levels are ADDED into the finer adjoint images below: on copies, so that a second backward of a retained
        # graph starts from the saved images again)
        gimgs = [gi.clone() for gi in gimgs[:-1]] + gimgs[-1:]
        dev = traj.device
        g = _f32c(g_loss.reshape(1))
        # the coarser levels' adjoint images into the finer ones, each in units of its own level's 1 / val^2 coefficient
        for lv in range(L - 1, 0, -1):
            h, w = ctx.sizes[lv - 1]
            _call('mpc_pool2_bwd_add', dev, _ptr(gimgs[lv]), ctypes.c_void_p(scals[lv].data_ptr() + 4 * C.SCAL_GCOEF), _ptr(gimgs[lv - 1]),
                  ctypes.c_void_p(scals[lv - 1].data_ptr() + 4 * C.SCAL_GCOEF), ctx.nimg, h, w)
        return _staged_bwd(cfg, shape, traj, ev, tr, flow_lut, state, gimgs[0], scals[0], g_field, g, ws), None, None, None, None, None


class _Marker:
    """Lives as long as the autograd context it is attached to (StaticFocusCalcFn, automatic mode)."""
    __slots__ = ('__weakref__',)


class StaticFocusPlan:
    """FocusLoss(static_shapes=True): `calc` + backward of ONE shape captured once into two HIP graphs (forward; backward)
    over buffers that never move, and replayed from then on -- what a B = 1 step costs on the host drops from two eager
    C-ABI calls with their allocations to two graph launches and three small copies.  The reference has no counterpart
    (PyTorch eager); the caller is unchanged (src/modules/trajectory_net.py:152-158).  Consequences of buffers that never
    move, all checked or documented: `misc_metadata['iwes']` is valid until the next `calc` of this shape; a backward must
    belong to the latest `calc` (checked); inputs are COPIED into the captured buffers every step (events only when the
    caller hands over a different tensor than last time)."""

    def __init__(self, cfg, B, M, Mp, n, dev, need_grad, traj, ev, tr, offs):
        p = self.plan = _plan(cfg, B, M, Mp, n, need_grad, offs is not None, dev)
        self.dev = dev
        # the offsets table of bucket-ordered events is an INPUT like the events: ingest hands over a fresh tensor with every
        # batch, so the plan owns a buffer of its own and the table is copied in every step (a few KB)
        self.offs = None
        if offs is not None:
            self.offs = torch.empty_like(_check_offsets(offs, cfg, p.shape, dev))
            self.offs.copy_(offs)
        self.traj, self.ev, self.tr = torch.empty_like(traj), torch.empty_like(ev), torch.empty_like(tr)
        self.ev_src, self.ev_version = None, -1
        self.ws = torch.empty(p.ws_bytes, dtype=torch.uint8, device=dev)
        self.buf = torch.empty(p.buf_floats, dtype=torch.float32, device=dev)
        self.blur = torch.empty(p.img_shape, dtype=torch.float32, device=dev)
        self.gout = torch.ones(1, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(_bwd_scratch_floats(p), dtype=torch.float32, device=dev) if need_grad else None
        # (pyramid_levels > 1: the pass is part of the captured forward, its workspace and level table belong to the plan)
        self.pyr_ws = torch.empty(p.pyr_bytes, dtype=torch.uint8, device=dev) if p.pyr_bytes else None
        self.pyr_scal = torch.empty((cfg.pyramid_levels, C.SCAL_COUNT), dtype=torch.float32, device=dev) if p.pyr_bytes else None
        self.g_traj = torch.empty_like(traj) if need_grad else None
        self.generation = 0
        self.pending = None              # weak reference to the marker of the latest calc that still waits for its backward (automatic mode)
        self.traj.copy_(traj); self.ev.copy_(ev); self.tr.copy_(tr)
        # one eager run on a side stream first: the library's one-time set-up must not fall into a capture
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._fwd()
            if need_grad:
                self._bwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # capture_error_mode='thread_local': only THIS thread's calls are held to the capture rules.  In the reference's training
        # process other threads use the device meanwhile (the DataLoader's pin_memory thread, src/modules/data_loading.py:141-142;
        # DDP's side streams and the RCCL watchdog, scripts/flow_training.py:125-130): in the default global mode an allocation of
        # theirs inside this window would invalidate the capture.
        self.g_fwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_fwd, capture_error_mode='thread_local'):
            self._fwd()
        self.g_bwd = None
        if need_grad:
            self.g_bwd = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_bwd, capture_error_mode='thread_local'):
                self._bwd()

    def _fwd(self):
        _focus_fwd_call(self.plan, self.dev, self.traj, self.ev, self.tr, self.buf, self.blur, self.ws, self.offs)
        if self.pyr_ws is not None:
            self.plan.pyramid(self.dev, self.buf, None, self.pyr_ws, self.pyr_scal)

    def _bwd(self):
        _focus_bwd_call(self.plan, self.dev, self.traj, self.ev, self.tr, self.buf, self.ws, self.offs, self.gout, self.scratch, self.g_traj)


class AutoPlanFailed(RuntimeError):
    """Automatic static shapes: the plan of a shape could not be captured (FocusLoss.calc then stays on the eager path)."""


class StaticFocusCalcFn(torch.autograd.Function):
    """FocusCalcFn replayed from the HIP graphs of a StaticFocusPlan."""

    @staticmethod
    def plan_key(trajectories, events, cfg, num_pos, event_offsets):
        """The key of the plan a calc of these inputs would use (shape only: every input is copied in)."""
        B, M = int(events.shape[0]), int(events.shape[1])
        Mp = int(num_pos) if cfg.polarity_split else M
        return (B, M, Mp, int(trajectories.shape[2]), bool(trajectories.requires_grad), trajectories.device.index, event_offsets is not None)

    @staticmethod
    def plan_busy(plans, key):
        """True while the latest calc of this plan still waits for its backward (its autograd context is alive and has not run):
        the captured buffers hold that step, another calc of the same shape must not replay over them."""
        sp = plans.get(key)
        return sp is not None and sp.pending is not None and sp.pending() is not None

    @staticmethod
    def forward(ctx, trajectories, events, t_ref, cfg: PathConfig, num_pos: int, event_offsets, plans: dict, auto: bool = False):
        B, M, Mp, n, dev, traj, ev, tr = _calc_inputs(trajectories, events, t_ref, cfg, num_pos)
        if knn_is_wide(n):
            raise _wide_limit('static_shapes=True', n)
        need_grad = trajectories.requires_grad
        key = StaticFocusCalcFn.plan_key(trajectories, events, cfg, num_pos, event_offsets)
        sp = plans.get(key)
        if sp is None:
            if len(plans) >= 8:              # every shape holds its buffers: keep the set small
                plans.pop(next(iter(plans)))
            if auto:
                # nobody asked for a capture: whatever goes wrong while the plan is built (a capture error, no memory for the
                # plan's buffers) must not reach the training step -- the caller takes the eager path for this shape from now on
                try:
                    sp = StaticFocusPlan(cfg, B, M, Mp, n, dev, need_grad, traj, ev, tr, event_offsets)
                except Exception as e:          # noqa: BLE001
                    raise AutoPlanFailed(f'{type(e).__name__}: {e}') from e
                plans[key] = sp
            else:
                sp = plans[key] = StaticFocusPlan(cfg, B, M, Mp, n, dev, need_grad, traj, ev, tr, event_offsets)
        sp.traj.copy_(traj)
        if sp.ev_src is None or sp.ev_src() is not events or events._version != sp.ev_version:
            sp.ev.copy_(ev)                 # a new batch (or one modified in place): copied once
            sp.ev_src, sp.ev_version = weakref.ref(events), events._version
        sp.tr.copy_(tr)
        if event_offsets is not None:
            sp.offs.copy_(_check_offsets(event_offsets, cfg, sp.plan.shape, dev))
        sp.generation += 1
        ctx.sp, ctx.gen = sp, sp.generation
        ctx.set_materialize_grads(False)
        sp.g_fwd.replay()
        o = sp.plan.o['scal'][0]
        out = sp.buf[o:o + 3].clone()
        loss, focus, smooth = out[C.SCAL_LOSS], out[C.SCAL_FOCUS], out[C.SCAL_SMOOTH]
        ctx.mark_non_differentiable(focus, smooth)
        # (the automatic mode keeps the reference's semantics: the images are the caller's own copy, and the plan is marked busy until
        # this step's backward has run or its graph is dropped -- FocusLoss.calc then takes the eager path for a second calc)
        sp.pending = None
        ctx.redo = None
        if auto and need_grad:
            ctx.marker = _Marker()
            sp.pending = weakref.ref(ctx.marker)
            # (what an eager step needs, should this backward come after the plan has moved on: references, no copies)
            ctx.redo = (traj, ev, tr, cfg, num_pos, event_offsets)
        return loss, focus, smooth, (sp.blur.clone() if auto else sp.blur.detach())

    @staticmethod
    def backward(ctx, g_loss, g_focus, g_smooth, g_iwes):
        if g_loss is None:
            return None, None, None, None, None, None, None, None
        sp = ctx.sp
        if ctx.gen == sp.generation:
            sp.pending = None
        elif ctx.redo is not None:
            # automatic mode, and the captured buffers hold a later calc of this shape (a second backward of a retained graph
            # after the next step): the caller never asked for static shapes, so it gets what the eager path gives -- the
            # step once more, eagerly, from the inputs this context kept
            traj, ev, tr, cfg, num_pos, offs = ctx.redo
            with torch.enable_grad():
                t = traj.detach().requires_grad_(True)
                out = FocusCalcFn.apply(t, ev, tr, cfg, num_pos, offs)
                (g,) = torch.autograd.grad(out[0], t, g_loss.reshape(()).to(out[0].dtype))
            return g, None, None, None, None, None, None, None
        if ctx.gen != sp.generation:
            raise RuntimeError('FocusLoss(static_shapes=True): this backward belongs to an earlier calc() of the same shape; the '
                               'captured buffers hold the latest one (call backward before the next calc, or use static_shapes=False)')
        sp.gout.copy_(g_loss.reshape(1))
        sp.g_bwd.replay()
        return sp.g_traj.clone(), None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------
# autograd: stage-level ops (used by tests, the bench's event-path figure and other callers)
# ------------------------------------------------------------------------------------------
class EventFocusFn(torch.autograd.Function):
    """A6-A9 with the LUT given: flow_lut -> (focus_loss, iwes_blurred, iwes_raw)."""

    @staticmethod
    def forward(ctx, flow_lut, events, t_ref, cfg: PathConfig, num_pos: int):
        _require_gpu(flow_lut, 'flow_lut')
        B, M, Mp = _check_events(events, cfg, num_pos)
        dev = flow_lut.device
        lut = _f32c(flow_lut.detach())
        ev = _f32c(events.detach())
        tr = _f32c(t_ref.detach().to(dev))
        need_grad = flow_lut.requires_grad
        shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=0 if need_grad else C.F_NO_BWD_RECORDS)
        ws = alloc_workspace(shape, dev)
        iwe_pyramid_check(cfg, shape, dev)
        raw = event_splat_fwd(shape, ev, lut, tr, ws)
        blur, gimg = contrast_fwd(shape, raw, ws, need_grad)
        scal = finalize(shape, 0, 0, 0.0, ws, dev)
        if cfg.pyramid_levels > 1:
            iwe_pyramid_pass(shape, cfg.pyramid_levels, raw, gimg, scal)
        ctx.shape, ctx.ws = shape, ws
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ev, tr, lut, gimg, scal)
        focus = scal[C.SCAL_FOCUS].clone()
        ctx.mark_non_differentiable(blur, raw)
        return focus, blur, raw

    @staticmethod
    def backward(ctx, g_focus, g_blur, g_raw):
        ev, tr, lut, gimg, scal = ctx.saved_tensors
        if g_focus is None:
            return None, None, None, None, None
        g = _f32c(g_focus.reshape(1))
        g_lut = torch.empty_like(lut)
        event_splat_bwd(ctx.shape, ev, lut, tr, gimg, scal, g, g_lut, None, ctx.ws)
        return g_lut, None, None, None, None


def pe_table_supported(cfg, events, num_pos, k, samples):
    """Do the table kernels (mpc_pe_table_*) serve this batch with a [samples + 1, k] table?  The library's answer: the rule --
    k, num_bins, the LDS the table's accumulators take -- lives there only."""
    if not (torch.is_tensor(events) and events.is_cuda):
        return False
    B, M, Mp = _check_events(events, cfg, num_pos)
    shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
    return _query('mpc_pe_table_supported', events.device, ctypes.byref(shape), int(k), int(samples)) == 1


def _pe_tail(cfg, shape, rows, tr, ws, need_grad, field=None):
    """What every fused per-event node runs on its warped rows: mpc_event_splat_fwd (MPC_F_NO_WARP) -> mpc_contrast_fwd
    [-> `field` = (entry point, tile rows, phim [nbm, k], k): the smoothness field -> mpc_lut_smooth] -> mpc_finalize ->
    (blurred images, adjoint images or None, gradient of the field or None, scalars)."""
    raw = event_splat_fwd(shape, rows, None, tr, ws)
    blur, gimg = contrast_fwd(shape, raw, ws, need_grad)
    g_field, s_nimg = None, 0
    pyr = cfg.pyramid_levels > 1
    if field is not None:
        name, c_rows, pm, k = field
        nbm = pm.shape[0]
        s_nimg = shape.B * nbm
        fld = torch.empty((s_nimg, shape.hq, shape.wq, 2), dtype=torch.float32, device=rows.device)
        _call(name, rows.device, _ptr(c_rows), _ptr(pm), _ptr(fld), shape.B, shape.hq * shape.wq, k, nbm)
        g_field = lut_smooth(shape, fld, s_nimg, 2, cfg.smooth_weight, ws, need_grad)
    scal = finalize(shape, s_nimg, 2 if s_nimg else 0, cfg.smooth_weight if s_nimg else 0.0, ws, rows.device)
    if pyr:
        iwe_pyramid_pass(shape, cfg.pyramid_levels, raw, gimg, scal)
    return blur, gimg, g_field, scal


def _pe_outputs(ctx, scal, blur):
    """(loss, focus, smooth, blur) of a fused per-event node from the scalars of _pe_tail: one copy of three floats."""
    out = scal[:3].clone()
    loss, focus, smooth = out[C.SCAL_LOSS], out[C.SCAL_FOCUS], out[C.SCAL_SMOOTH]
    ctx.mark_non_differentiable(focus, smooth, blur)
    return loss, focus, smooth, blur


def _pe_fwd(cfg, shape, ev, coef_rows, ph, k, tr, ws, need_grad, tab=None, field=None):
    """The per-event forward core: mpc_pe_warp (`tab` [S + 1, k]: mpc_pe_table_warp) -> _pe_tail -> (warped rows, *its results)."""
    rows = torch.empty_like(ev)
    if shape.B * shape.M > 0 and tab is not None:
        _call('mpc_pe_table_warp', ev.device, ctypes.byref(shape), _ptr(ev), _ptr(coef_rows), _ptr(tab), tab.shape[0] - 1, k, _ptr(tr), _ptr(rows))
    elif shape.B * shape.M > 0:               # (an empty tensor has no pointer to hand over)
        _call('mpc_pe_warp', ev.device, ctypes.byref(shape), _ptr(ev), _ptr(coef_rows), _ptr(ph), k, _ptr(tr), _ptr(rows))
    return (rows,) + _pe_tail(cfg, shape, rows, tr, ws, need_grad, field)


def _pe_ordered_offsets(offsets, cfg, shape, k, dev):
    """The checked offsets table when the ordered backward will serve this shape, else None."""
    # bucket-ordered events: the backward accumulates per LUT strip in LDS (no global atomics) where a strip's accumulators fit
    # (the library says whether the ordered backward serves this shape -- one copy of the rule; where it does not, an offsets
    # table is simply not used: the atomic backward needs none)
    if offsets is None or _query('mpc_pe_grad_ordered_supported', dev, ctypes.byref(shape), k) != 1:
        return None
    return _check_offsets(offsets, cfg, shape, dev)


def _pe_pos_grad(shape, k, rows, offs, ph, tr, gimg, scal, go, tab=None, gpos=None):
    """d objective / d tile coefficients through the warped positions, as partial results [split, B*hq*wq, 2k] for the caller to sum:
    the ordered kernel on bucket-ordered rows (`offs`), the atomic kernel (split = 1) otherwise.  `tab` [S + 1, k]: the table
    instantiations of the same kernels, which also leave every row's unscaled position gradient in `gpos` [B, M, 2] (or None)."""
    dev = rows.device
    n = shape.B * shape.hq * shape.wq
    if offs is not None:
        # (a few workgroups per (sample, LUT strip), each with a share of the strip's row ranges and a partial result)
        split = max(1, min(16, 512 // max(1, shape.B * _lut_strips(shape, dev))))
        gp = torch.empty((split, n, 2 * k), dtype=torch.float32, device=dev)
        if tab is not None:
            rc = _call('mpc_pe_table_grad_ordered', dev, ctypes.byref(shape), _ptr(rows), _ptr(offs), _ptr(tab), tab.shape[0] - 1, k, _ptr(tr),
                       _ptr(gimg), _ptr(scal), _ptr(go), _ptr(gp), split, _ptr(gpos), accept=(C.E_UNSUPPORTED,))
        else:
            rc = _call('mpc_pe_grad_ordered', dev, ctypes.byref(shape), _ptr(rows), _ptr(offs), _ptr(ph), k, _ptr(tr), _ptr(gimg), _ptr(scal),
                       _ptr(go), _ptr(gp), split, accept=(C.E_UNSUPPORTED,))
        if rc == 0:
            return gp
        # (unsupported after all: the atomic backward below serves every shape)
    gp = torch.empty((1, n, 2 * k), dtype=torch.float32, device=dev)
    if tab is not None:
        _call('mpc_pe_table_grad', dev, ctypes.byref(shape), _ptr(rows), _ptr(tab), tab.shape[0] - 1, k, _ptr(tr), _ptr(gimg), _ptr(scal),
              _ptr(go), _ptr(gp), _ptr(gpos))
        return gp
    _call('mpc_pe_grad', dev, ctypes.byref(shape), _ptr(rows), _ptr(ph), k, _ptr(tr), _ptr(gimg), _ptr(scal), _ptr(go), _ptr(gp))
    return gp


class PerEventBasisFocusFn(torch.autograd.Function):
    """UNPINNED extension (FocusLoss.calc_per_event_basis), fused form: tile coefficients coef_rows [B*hq*wq, 2k] (differentiable),
    events [B, M, 6], phi [B, M, k] = basis(t_ref) - basis(t_event) -> (focus_loss, iwes_blurred).
    Forward: mpc_pe_warp -> mpc_event_splat_fwd (MPC_F_NO_WARP) -> mpc_contrast_fwd -> mpc_finalize; backward: mpc_pe_grad."""

    @staticmethod
    def forward(ctx, coef_rows, events, phi, t_ref, cfg: PathConfig, num_pos: int, offsets=None):
        _require_gpu(coef_rows, 'coef_rows')
        B, M, Mp = _check_events(events, cfg, num_pos)
        dev = coef_rows.device
        cr = _f32c(coef_rows.detach())
        ev = _f32c(events.detach())
        ph = _f32c(phi.detach()) if phi is not None else None       # None: the polynomial basis, worked out in the kernels
        k = int(ph.shape[-1]) if ph is not None else int(coef_rows.shape[1]) // 2
        tr = _f32c(t_ref.detach().to(dev))
        need_grad = coef_rows.requires_grad
        shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
        iwe_pyramid_check(cfg, shape, dev)
        if tuple(cr.shape) != (B * shape.hq * shape.wq, 2 * k) or (ph is not None and tuple(ph.shape) != (B, M, k)) or (ph is None and k > 8):
            raise ValueError(f'coef_rows {tuple(cr.shape)} / phi do not match [B*hq*wq, 2k] / [B, M, k] (k <= 8 without phi)')
        ws = alloc_workspace(shape, dev)
        rows, blur, gimg, _, scal = _pe_fwd(cfg, shape, ev, cr, ph, k, tr, ws, need_grad)
        ctx.shape, ctx.k = shape, k
        offs = _pe_ordered_offsets(offsets, cfg, shape, k, dev)
        ctx.has_offs = offs is not None
        ctx.set_materialize_grads(False)
        ctx.has_phi = ph is not None
        # (the table goes through save_for_backward: autograd's version check then catches a refill between forward and backward)
        ctx.save_for_backward(rows, ph if ph is not None else tr, tr, gimg, scal, offs if offs is not None else tr)
        ctx.mark_non_differentiable(blur)
        return scal[C.SCAL_FOCUS].clone(), blur

    @staticmethod
    def backward(ctx, g_focus, g_blur):
        rows, ph, tr, gimg, scal, offs = ctx.saved_tensors
        if not ctx.has_phi:
            ph = None
        if g_focus is None:
            return None, None, None, None, None, None, None
        go = _f32c(g_focus.reshape(1))
        gp = _pe_pos_grad(ctx.shape, ctx.k, rows, offs if ctx.has_offs else None, ph, tr, gimg, scal, go)
        return (gp.sum(0) if gp.shape[0] > 1 else gp[0]), None, None, None, None, None, None


class PerEventBasisCalcFn(torch.autograd.Function):
    """UNPINNED extension (FocusLoss.calc_per_event_basis), the whole step as ONE autograd node of library calls (round 6):
    dense coefficient grid -> tile rows -> per-event warp -> vote -> blur + objective [-> smoothness field -> Charbonnier term]
    -> scalars, and back: position gradient per LUT strip -> (+ smoothness adjoint) -> dense gradient.  Rounds 4-5 spelt the dense <->
    per-tile operators and the smoothness field in torch (TileCoeffRowsFn, BasisFieldFn, LutSmoothFn below: kept for the unfused
    cross-check): two dozen operators around 0.30 ms of kernels, and the step was bound by the host (0.74-0.97 ms at the DSEC batch
    shape).  Returns (loss, focus, smooth, iwes_blurred); differentiable w.r.t. coeff_grid through `loss`.

    `table` [S + 1, k] (basis_type='table'; phi must be None): the kernels interpolate the basis from it at every event's time
    (mpc_pe_table_*), and the node is differentiable w.r.t. the table as well -- through the events by mpc_pe_table_basis_grad (one
    streaming pass over 8 bytes per event of position gradients that the coefficient backward leaves behind), through the
    smoothness term by returning the gradient of `phim` (mpc_pe_field_basis_grad), which torch chains into the table through
    utils.table_basis_values.  With no table the node runs the calls it ran before."""

    @staticmethod
    def forward(ctx, coeff_grid, events, phi, phim, t_ref, cfg: PathConfig, num_pos: int, offsets, k: int, tile: int, table=None):
        _require_gpu(coeff_grid, 'coeff_grid')
        B, M, Mp = _check_events(events, cfg, num_pos)
        dev = coeff_grid.device
        cg, cg_dt = _net(coeff_grid)                                # (fp16 / bf16 grids are read as they are: no .float() copy)
        ev = _f32c(events.detach())
        ph = _f32c(phi.detach()) if phi is not None else None       # None: the polynomial basis, worked out in the kernels
        pm = _f32c(phim.detach()) if phim is not None else None     # [nb, k]: basis(t_ref) - basis(bin mid-times), or None: no smoothness term
        tr = _f32c(t_ref.detach().to(dev))
        need_grad = coeff_grid.requires_grad
        tab = None
        if table is not None:
            _require_gpu(table, 'basis_table')
            tab = _f32c(table.detach())
            if ph is not None or tab.dim() != 2 or tab.shape[1] != k or tab.shape[0] < 2:
                raise ValueError(f'basis_table {tuple(table.shape)} is not [samples + 1, {k}] (and takes no phi)')
            need_grad = need_grad or table.requires_grad or (phim is not None and phim.requires_grad)
        Bc, S, c2, H, W = cg.shape
        shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
        iwe_pyramid_check(cfg, shape, dev)
        G = shape.hq * shape.wq
        if Bc != B or c2 != 2 * k or (ph is not None and tuple(ph.shape) != (B, M, k)) or (ph is None and k > 8):
            raise ValueError(f'coeff_grid {tuple(cg.shape)} / phi do not match [B, S, 2k, H, W] / [B, M, k] (k <= 8 without phi)')
        c_rows = torch.empty((B * G, 2 * k), dtype=torch.float32, device=dev)
        _call('mpc_pe_tile_rows_dt', dev, _ptr(cg), cg_dt, _ptr(c_rows), B, S, c2, H, W, tile, label='mpc_pe_tile_rows')
        ws = alloc_workspace(shape, dev)
        field = ('mpc_pe_basis_field', c_rows, pm, k) if pm is not None and cfg.smooth_weight > 0 else None
        rows, blur, gimg, g_field, scal = _pe_fwd(cfg, shape, ev, c_rows, ph, k, tr, ws, need_grad, tab, field)
        offs = _pe_ordered_offsets(offsets, cfg, shape, k, dev)
        ctx.shape, ctx.k, ctx.tile, ctx.grid_shape, ctx.grid_dtype = shape, k, tile, (B, S, c2, H, W), cg.dtype
        ctx.has = (ph is not None, pm is not None and g_field is not None, offs is not None)
        ctx.has_tab = tab is not None
        ctx.set_materialize_grads(False)
        none = tr
        # (the tile rows are kept for the table route only: both table gradients are products with them)
        ctx.save_for_backward(rows, ph if ph is not None else none, tr, gimg if gimg is not None else none, scal,
                              offs if offs is not None else none, g_field if g_field is not None else none, pm if pm is not None else none,
                              tab if tab is not None else none, c_rows if tab is not None else none)
        return _pe_outputs(ctx, scal, blur)

    @staticmethod
    def backward(ctx, g_loss, g_focus, g_smooth, g_blur):
        if g_loss is None:
            return (None,) * 11
        rows, ph, tr, gimg, scal, offs, g_field, pm, tab, c_rows = ctx.saved_tensors
        has_phi, has_smooth, has_offs = ctx.has
        ph = ph if has_phi else None
        shape, k = ctx.shape, ctx.k
        B, S, c2, H, W = ctx.grid_shape
        G = shape.hq * shape.wq
        dev = rows.device
        go = _f32c(g_loss.reshape(1))
        g_table = g_phim = gpos = None
        if ctx.has_tab:
            if ctx.needs_input_grad[10]:
                gpos = torch.empty((shape.B, shape.M, 2), dtype=torch.float32, device=dev)
            gp = _pe_pos_grad(shape, k, rows, offs if has_offs else None, None, tr, gimg, scal, go, tab, gpos)
            if gpos is not None:
                ns = tab.shape[0] - 1
                acc = torch.empty(((ns + 2) * k,), dtype=torch.int64, device=dev)
                g_table = torch.empty_like(tab)
                _call('mpc_pe_table_basis_grad', dev, ctypes.byref(shape), _ptr(rows), _ptr(gpos), _ptr(c_rows), ns, k, _ptr(tr), _ptr(scal),
                      _ptr(go), _ptr(acc), _ptr(g_table))
            if has_smooth and ctx.needs_input_grad[3]:
                nbm = pm.shape[0]
                part = torch.empty((nbm * 64 * k,), dtype=torch.float64, device=dev)
                g_phim = torch.empty_like(pm)
                _call('mpc_pe_field_basis_grad', dev, _ptr(g_field), _ptr(c_rows), _ptr(go), _ptr(part), _ptr(g_phim), B, G, k, nbm)
        else:
            gp = _pe_pos_grad(shape, k, rows, offs if has_offs else None, ph, tr, gimg, scal, go)
        g_rows = torch.empty((B * G, 2 * k), dtype=torch.float32, device=dev)
        nb = pm.shape[0] if has_smooth else 0
        _call('mpc_pe_rows_grad_finish', dev, _ptr(gp), gp.shape[0], _ptr(g_field) if has_smooth else None, _ptr(pm) if has_smooth else None,
              _ptr(go), _ptr(g_rows), B, G, k, max(nb, 1))
        g_grid = torch.empty(ctx.grid_shape, dtype=ctx.grid_dtype, device=dev)          # (in the grid's dtype; every element is written)
        _call('mpc_pe_tile_rows_bwd_dt', dev, _ptr(g_rows), _ptr(g_grid), _DT_CODE[ctx.grid_dtype], B, S, c2, H, W, ctx.tile,
              label='mpc_pe_tile_rows_bwd')
        return (g_grid, None, None, g_phim) + (None,) * 6 + (g_table,)


PEC_BASIS = {'BEZIER': 0, 'POLYNOMIAL': 1, 'TABLE': 2, 'BSPLINE': 3}        # include/mpcmax.h: MPC_PEC_*
PEC_ROWS_GRAD_TAP = None       # diagnostics (tests): a list that receives a copy of every grad_rows [B*G, 2d] PerEventCurvesFn computes


def _pec_shape(cfg, events, num_pos):
    B, M, Mp = _check_events(events, cfg, num_pos)
    return make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)


def pec_supported(cfg, events, num_pos, d, curve_type, samples=0):
    """mpc_pec_supported for this batch: 0 = the curve kernels (csrc/pe_curves.hip) do not serve it, bit 0 = they do, bit 1 = the
    row gradient also takes an offsets table.  The library's answer: the limits live there only."""
    if not (torch.is_tensor(events) and events.is_cuda) or curve_type not in PEC_BASIS:
        return 0
    shape = _pec_shape(cfg, events, num_pos)
    return _query('mpc_pec_supported', events.device, ctypes.byref(shape), int(d), PEC_BASIS[curve_type], int(samples))


class PerEventCurvesFn(torch.autograd.Function):
    """UNPINNED extension (FocusLoss.calc_per_event_curves): the per-event continuous-time warp along RAFT-spline curves as ONE
    autograd node of library calls on the current stream (csrc/pe_curves.hip):
    head rows (mpc_pec_head_rows) -> warp (mpc_pec_warp) -> vote (mpc_event_splat_fwd, MPC_F_NO_WARP) -> blur + objective
    (mpc_contrast_fwd) [-> field (mpc_pec_field) -> Charbonnier term (mpc_lut_smooth)] -> scalars (mpc_finalize), and back:
    mpc_event_pos_grad -> mpc_pec_rows_grad [-> mpc_pec_field_adjoint] -> mpc_pec_head_rows_bwd.
    params [B, 2d, h, w] (x channels first), up_mask [B, 576, h, w] or None, phim [nbm, d] or None (no smoothness term), table
    [S + 1, d] or None.  Returns (loss, focus, smooth, iwes_blurred); differentiable w.r.t. params and up_mask through `loss`.
    A table that requires grad trains as well: through the events by mpc_pec_table_basis_grad (one streaming pass over the warped
    records, the position gradients the backward has anyway and the tile rows; Q33.30 sums, bitwise reproducible in either event
    layout), through the smoothness term by returning the gradient of `phim` (mpc_pec_field_basis_grad), which torch chains into
    the table through utils.table_basis_values.  The tile rows are kept for that only: with a constant table (and phim) the node
    makes the calls it made before the table could train, the same launches and the same bits.
    No host synchronisation.  The position gradient is taken UNSCALED (a `scal` of ones) and the loss scale applied after the
    fixed-point sums, as k_pe_accum does: the sums' resolution does not depend on grad_out."""

    @staticmethod
    def forward(ctx, params, up_mask, events, t_ref, phim, cfg: PathConfig, num_pos: int, offsets, curve_type: str, table, scale: float,
                tile: int, orders_per_pass: int = 0):
        _require_gpu(params, 'params')
        B, M, Mp = _check_events(events, cfg, num_pos)
        dev = params.device
        p = _f32c(params.detach())
        m, m_dt = None, C.DT_F32
        if up_mask is not None:
            _require_gpu(up_mask, 'up_mask')
            m, m_dt = _net(up_mask)                   # (an fp16 / bf16 mask is read as it is: no .float() copy)
        ev = _f32c(events.detach())
        pm = _f32c(phim.detach()) if phim is not None else None
        tr = _f32c(t_ref.detach().to(dev))
        tab = None
        if table is not None:
            _require_gpu(table, 'basis_table')
            tab = _f32c(table.detach())
        Bp, c2, h, w = p.shape
        d, kind, S = c2 // 2, PEC_BASIS[curve_type], (tab.shape[0] - 1 if tab is not None else 0)
        shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
        iwe_pyramid_check(cfg, shape, dev)
        hq, wq = shape.hq, shape.wq
        G = hq * wq
        grid = (8 * h // tile, 8 * w // tile) if m is not None else (h, w)
        if Bp != B or c2 != 2 * d or grid != (hq, wq) or (m is not None and tuple(m.shape) != (B, 576, h, w)) or \
                (tab is not None and (tab.dim() != 2 or tab.shape[1] != d)) or (pm is not None and (pm.dim() != 2 or pm.shape[1] != d)):
            raise ValueError(f'params {tuple(p.shape)} / up_mask / basis_table / phim do not match [B={B}, 2d, h, w] with the tile grid {(hq, wq)}')
        sup = _query('mpc_pec_supported', dev, ctypes.byref(shape), d, kind, S)
        if not sup & 1:
            raise ValueError(f'the curve kernels do not serve d={d}, {curve_type}, samples={S}, num_bins={cfg.num_bins} (mpc_pec_supported)')
        need_grad = params.requires_grad or (up_mask is not None and up_mask.requires_grad)
        # (inputs 9 and 4: the table and phim -- a table that trains reaches the loss through both)
        basis_trains = (tab is not None and ctx.needs_input_grad[9]) or (pm is not None and ctx.needs_input_grad[4])
        need_grad = need_grad or basis_trains
        c_rows = torch.empty((B * G, 2 * d), dtype=torch.float32, device=dev)
        _call('mpc_pec_head_rows_dt', dev, _ptr(p), _ptr(m), m_dt, float(scale), int(tile), _ptr(c_rows), B, d, h, w, label='mpc_pec_head_rows')
        ws = alloc_workspace(shape, dev)
        rows = torch.empty_like(ev)
        if B * M > 0:                                 # (an empty tensor has no pointer to hand over)
            _call('mpc_pec_warp', dev, ctypes.byref(shape), _ptr(ev), _ptr(c_rows), kind, d, _ptr(tab), S, _ptr(tr), _ptr(rows))
        field = ('mpc_pec_field', c_rows, pm, d) if pm is not None and cfg.smooth_weight > 0 and pm.shape[0] > 0 else None
        blur, gimg, g_field, scal = _pe_tail(cfg, shape, rows, tr, ws, need_grad, field)
        offs = _check_offsets(offsets, cfg, shape, dev) if (offsets is not None and sup & 2) else None
        ctx.shape, ctx.dims = shape, (B, d, h, w, kind, S, float(scale), int(tile), int(orders_per_pass))
        ctx.has = (m is not None, g_field is not None, offs is not None, tab is not None)
        ctx.set_materialize_grads(False)
        none = tr
        ctx.save_for_backward(p, m if m is not None else none, rows, tr, gimg if gimg is not None else none, scal,
                              offs if offs is not None else none, g_field if g_field is not None else none,
                              pm if pm is not None else none, tab if tab is not None else none, c_rows if basis_trains else none)
        return _pe_outputs(ctx, scal, blur)

    @staticmethod
    def backward(ctx, g_loss, g_focus, g_smooth, g_blur):
        if g_loss is None:
            return (None,) * 13
        p, m, rows, tr, gimg, scal, offs, g_field, pm, tab, c_rows = ctx.saved_tensors
        has_mask, has_smooth, has_offs, has_tab = ctx.has
        shape = ctx.shape
        B, d, h, w, kind, S, scale, tile, opp = ctx.dims
        G = shape.hq * shape.wq
        dev = rows.device
        go = _f32c(g_loss.reshape(1))
        gpos = None
        if shape.B * shape.M > 0:
            unit = torch.ones(C.SCAL_COUNT, dtype=torch.float32, device=dev)
            gpos = event_pos_grad(shape, rows, tr, gimg, unit, None)
        g_rows = torch.empty((B * G, 2 * d), dtype=torch.float32, device=dev)
        _call('mpc_pec_rows_grad', dev, ctypes.byref(shape), _ptr(rows) if gpos is not None else None, _ptr(offs) if has_offs else None, _ptr(gpos),
              kind, d, _ptr(tab) if has_tab else None, S, _ptr(tr), _ptr(scal), _ptr(go), opp, _ptr(g_rows))
        if has_smooth:
            _call('mpc_pec_field_adjoint', dev, _ptr(g_field), _ptr(pm), _ptr(go), _ptr(g_rows), B, G, d, pm.shape[0])
        g_table = g_phim = None
        if has_tab and ctx.needs_input_grad[9]:
            acc = torch.empty(((S + 2) * d,), dtype=torch.int64, device=dev)
            g_table = torch.empty_like(tab)
            _call('mpc_pec_table_basis_grad', dev, ctypes.byref(shape), _ptr(rows) if gpos is not None else None, _ptr(gpos), _ptr(c_rows), d, S,
                  _ptr(tr), _ptr(scal), _ptr(go), _ptr(acc), _ptr(g_table))
        if has_smooth and ctx.needs_input_grad[4]:
            nbm = pm.shape[0]
            part = torch.empty((nbm * 64 * d,), dtype=torch.float64, device=dev)
            g_phim = torch.empty_like(pm)
            _call('mpc_pec_field_basis_grad', dev, _ptr(g_field), _ptr(c_rows), _ptr(go), _ptr(part), _ptr(g_phim), B, G, d, nbm)
        if PEC_ROWS_GRAD_TAP is not None:
            PEC_ROWS_GRAD_TAP.append(g_rows.clone())
        gp = torch.empty((B, 2 * d, h, w), dtype=torch.float32, device=dev)
        gm = ws = None
        if has_mask:
            gm = torch.empty((B, 576, h, w), dtype=m.dtype, device=dev)                # (in the mask's dtype; every element is written)
            ws = torch.empty(max(_query('mpc_pec_head_rows_bwd_workspace_bytes', dev, B, d, h, w, tile), 256), dtype=torch.uint8, device=dev)
        _call('mpc_pec_head_rows_bwd_dt', dev, _ptr(g_rows), _ptr(p), _ptr(m) if has_mask else None, _DT_CODE[m.dtype] if has_mask else C.DT_F32,
              scale, tile, _ptr(gp), _ptr(gm), B, d, h, w, _ptr(ws), label='mpc_pec_head_rows_bwd')
        return (gp, gm, None, None, g_phim) + (None,) * 4 + (g_table,) + (None,) * 3


class TileCoeffRowsFn(torch.autograd.Function):
    """coeff_grid [B, S, 2k, H, W] -> the coefficients at the tile centres (offset tile // 2, row-major: trajectories.py:3-52),
    scales summed, one row per tile: [B*hq*wq, 2k].  One autograd node with a strided copy each way instead of the half dozen
    view / sum / permute nodes of the plain-torch spelling (the per-event step is bound by the host)."""

    @staticmethod
    def forward(ctx, coeff_grid, tile):
        ctx.shape_in, ctx.tile = tuple(coeff_grid.shape), int(tile)
        cs = coeff_grid[:, :, :, tile // 2::tile, tile // 2::tile]
        cs = cs[:, 0] if cs.shape[1] == 1 else cs.sum(1)                      # [B, 2k, hc, wc]
        B, c2, hc, wc = cs.shape
        hq, wq = -(-coeff_grid.shape[3] // tile), -(-coeff_grid.shape[4] // tile)
        if (hc, wc) != (hq, wq):
            # (0 < H % tile <= tile // 2: the centre of the last row of cells lies outside the image -- zero coefficients, as
            # k_tile_rows writes them)
            cs = torch.nn.functional.pad(cs, (0, wq - wc, 0, hq - hc))
        return cs.permute(0, 2, 3, 1).reshape(B * hq * wq, c2)

    @staticmethod
    def backward(ctx, g):
        B, S, c2, H, W = ctx.shape_in
        t = ctx.tile
        out = torch.zeros(ctx.shape_in, dtype=g.dtype, device=g.device)
        view = out[:, :, :, t // 2::t, t // 2::t]
        hq, wq = -(-H // t), -(-W // t)
        gc = g.reshape(B, hq, wq, c2)[:, :view.shape[3], :view.shape[4]]      # (cells without a centre in the image: dropped)
        view.copy_(gc.permute(0, 3, 1, 2)[:, None].expand_as(view))
        return out, None


class BasisFieldFn(torch.autograd.Function):
    """c_rows [B*G, 2k] (per tile: y orders, x orders), phim [nb, k] -> flow field at nb times [B*nb, hq, wq, 2] (the layout
    of LutSmoothFn): field[b, t, cell, d] = sum_j c[b, cell, d, j] phim[t, j].  One node, a small GEMM and a copy each way."""

    @staticmethod
    def forward(ctx, c_rows, phim, B, hq, wq):
        k = phim.shape[1]
        ctx.save_for_backward(phim)
        ctx.dims = (B, hq, wq, k)
        f = c_rows.reshape(B * hq * wq * 2, k) @ phim.t()                     # [B*G*2, nb]
        return f.view(B, hq * wq, 2, phim.shape[0]).permute(0, 3, 1, 2).reshape(B * phim.shape[0], hq, wq, 2)

    @staticmethod
    def backward(ctx, g):
        (phim,) = ctx.saved_tensors
        B, hq, wq, k = ctx.dims
        nb = phim.shape[0]
        gf = g.reshape(B, nb, hq * wq, 2).permute(0, 2, 3, 1).reshape(B * hq * wq * 2, nb)
        return (gf @ phim).view(B * hq * wq, 2 * k), None, None, None, None


class GatherRowsFn(torch.autograd.Function):
    """rows[idx] whose backward is index_add_ (float atomics) -- torch's own advanced-indexing backward sorts the indices
    (index_put_ with accumulate): tens of milliseconds for the 2.8 M events of a DSEC batch.  UNPINNED extension
    (FocusLoss.calc_per_event_basis); the gradient it returns is not bitwise reproducible."""

    @staticmethod
    def forward(ctx, rows, idx):
        ctx.save_for_backward(idx)
        ctx.n = rows.shape[0]
        return rows.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.zeros((ctx.n, g.shape[1]), dtype=g.dtype, device=g.device).index_add_(0, idx, g.contiguous()), None


def event_pos_grad(shape, rows, t_ref, gimg, scal, grad_out):
    """UNPINNED extension: d objective / d warped position per event row -> [B, M, 2] (mpc_event_pos_grad)."""
    B, M = rows.shape[0], rows.shape[1]
    g = torch.empty((B, M, 2), dtype=torch.float32, device=rows.device)
    _call('mpc_event_pos_grad', rows.device, ctypes.byref(shape), _ptr(rows), _ptr(t_ref), _ptr(gimg), _ptr(scal), _ptr(grad_out), _ptr(g))
    return g


class PrewarpedFocusFn(torch.autograd.Function):
    """UNPINNED extension (FocusLoss.calc_per_event_basis): A7-A9 on events whose positions are warped already.
    warped_pos [B, M, 2] (y, x; the differentiable input), events [B, M, 6] (columns 2.. = t, p, bin, valid as the loader
    writes them) -> (focus_loss, iwes_blurred).  Forward: the LDS-tiled vote of mpc_event_splat_fwd with MPC_F_NO_WARP;
    backward: mpc_event_pos_grad (one thread per row, no atomics)."""

    @staticmethod
    def forward(ctx, warped_pos, events, t_ref, cfg: PathConfig, num_pos: int):
        _require_gpu(warped_pos, 'warped_pos')
        B, M, Mp = _check_events(events, cfg, num_pos)
        dev = warped_pos.device
        rows = torch.cat((_f32c(warped_pos.detach()), _f32c(events.detach())[..., 2:]), dim=-1).contiguous()
        tr = _f32c(t_ref.detach().to(dev))
        need_grad = warped_pos.requires_grad
        shape = make_shape(cfg, B, M, Mp, 0, K=0, extra_flags=C.F_NO_WARP | C.F_NO_BWD_RECORDS)
        iwe_pyramid_check(cfg, shape, dev)
        ws = alloc_workspace(shape, dev)
        raw = event_splat_fwd(shape, rows, None, tr, ws)
        blur, gimg = contrast_fwd(shape, raw, ws, need_grad)
        scal = finalize(shape, 0, 0, 0.0, ws, dev)
        if cfg.pyramid_levels > 1:
            iwe_pyramid_pass(shape, cfg.pyramid_levels, raw, gimg, scal)
        ctx.shape = shape
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(rows, tr, gimg, scal)
        ctx.mark_non_differentiable(blur)
        return scal[C.SCAL_FOCUS].clone(), blur

    @staticmethod
    def backward(ctx, g_focus, g_blur):
        rows, tr, gimg, scal = ctx.saved_tensors
        if g_focus is None:
            return None, None, None, None, None
        return event_pos_grad(ctx.shape, rows, tr, gimg, scal, _f32c(g_focus.reshape(1))), None, None, None, None


class KnnLutFn(torch.autograd.Function):
    """A5: trajectories -> (flow_lut, flow_next or empty)."""

    @staticmethod
    def forward(ctx, trajectories, cfg: PathConfig):
        _require_gpu(trajectories, 'trajectories')
        traj = _f32c(trajectories.detach())
        B, _, n, _ = traj.shape
        shape = make_shape(cfg, B, 0, 0, n)
        ctx.wide = knn_is_wide(n)
        if ctx.wide:
            ws = None
            flow_lut, flow_next, state = knn_wide_fwd(cfg, shape, traj)      # (state: the merged index lists)
        else:
            ws = alloc_workspace(shape, traj.device)
            flow_lut, flow_next, state, _ = knn_lut_fwd(cfg, shape, traj, ws)
        ctx.shape, ctx.ws = shape, ws
        ctx.has_next = flow_next is not None
        ctx.save_for_backward(traj, state)
        if flow_next is None:
            flow_next = traj.new_zeros(0)
        return flow_lut, flow_next

    @staticmethod
    def backward(ctx, g_lut, g_next):
        traj, state = ctx.saved_tensors
        g_lut = _f32c(g_lut)
        g_next = _f32c(g_next) if ctx.has_next else None
        if ctx.wide:
            return knn_idx_bwd(ctx.shape, traj, g_lut, g_next, state), None
        return knn_lut_bwd(ctx.shape, traj, g_lut, g_next, state, ctx.ws), None


class LutSmoothFn(torch.autograd.Function):
    """A10: field [nimg, hq, wq, C] -> smooth_weight * smoothness."""

    @staticmethod
    def forward(ctx, field, cfg: PathConfig, weight: float):
        _require_gpu(field, 'field')
        f = _f32c(field.detach())
        nimg, hq, wq, Cch = f.shape
        if (hq, wq) != cfg.lut_grid:
            raise ValueError(f'field grid {(hq, wq)} does not match the LUT grid {cfg.lut_grid}')
        B = max(1, -(-nimg * Cch // (cfg.num_bins * cfg.num_tref * 2)))
        shape = make_shape(cfg, B, 0, 0, 0, K=0)
        ws = alloc_workspace(shape, f.device)
        g = lut_smooth(shape, f, nimg, Cch, weight, ws, field.requires_grad)
        # only the smoothness scalar of finalize is meaningful here (no contrast pass was run)
        scal = finalize(shape, nimg, Cch, weight, ws, f.device)
        ctx.save_for_backward(g)
        return scal[C.SCAL_SMOOTH].clone()

    @staticmethod
    def backward(ctx, g_out):
        (g,) = ctx.saved_tensors
        return scale(g, _f32c(g_out.reshape(1))), None, None


def _curve_basis_grad(G, R, layout, scale, B, d, T, sites):
    """grad_basis [T, d] fp32 of the three RAFT-spline nodes (csrc/curve_basis.hip: mpc_curve_basis_grad, two kernels behind the
    node's own backward launches): G the cotangent of the displacements, R the control points the sites evaluate, in the layout
    C.CBG_* of the node.  No host synchronisation; bitwise reproducible."""
    dev = G.device
    gb = torch.empty((T, d), dtype=torch.float32, device=dev)
    scratch = torch.empty(max(_query('mpc_curve_basis_grad_scratch_floats', dev, B, d, T, sites), 1), dtype=torch.float32, device=dev)
    _call('mpc_curve_basis_grad', dev, _ptr(G), _ptr(R), int(layout), float(scale), _ptr(gb), _ptr(scratch), B, d, T, sites)
    return gb


class CurveTrajFn(torch.autograd.Function):
    """Flow curves -> `trajectories` (BASELINE.json configs[3]): params [B, 2d, h, w] ((x, y) channel order,
    reference curves/polynomial.py:60-61), basis [T, d] on the device, tile centres [n, 2] (y, x) -> [B, T, n, 2], one kernel each
    way (csrc/curves.hip) instead of the einsum / stack / add chain of plain torch and its adjoints.  A basis matrix that requires
    grad (a learned basis that trains, routed here by basis_grad='fused') gets its gradient from `_curve_basis_grad` behind the
    backward kernel; only the gradients autograd asks for are computed."""

    @staticmethod
    def forward(ctx, params, basis, pos, scale: float):
        _require_gpu(params, 'params')
        B, c2, h, w = params.shape
        d, n, T = c2 // 2, h * w, basis.shape[0]
        dev = params.device
        p = _f32c(params.detach())
        bm = _f32c(basis.detach())
        ps = _f32c(pos.detach())
        traj = torch.empty((B, T, n, 2), dtype=torch.float32, device=dev)
        _call('mpc_curve_traj_fwd', dev, _ptr(p), _ptr(bm), _ptr(ps), float(scale), _ptr(traj), B, d, T, n)
        ctx.save_for_backward(bm, p if ctx.needs_input_grad[1] else None)
        ctx.dims = (B, d, T, n, h, w, float(scale))
        return traj

    @staticmethod
    def backward(ctx, g):
        bm, p = ctx.saved_tensors
        B, d, T, n, h, w, scale = ctx.dims
        g = _f32c(g)
        gp = gb = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty((B, 2 * d, h, w), dtype=torch.float32, device=g.device)
            _call('mpc_curve_traj_bwd', g.device, _ptr(g), _ptr(bm), scale, _ptr(gp), B, d, T, n)
        if p is not None:
            gb = _curve_basis_grad(g, p, C.CBG_PLAIN, scale, B, d, T, n)
        return gp, gb, None, None


class CvxCurveTrajFn(torch.autograd.Function):
    """The RAFT-spline output head -> `trajectories`: control points on the 1/8 grid params [B, 2d, h, w] ((x, y) channel order) and
    the convex-upsampling logits up_mask [B, 576, h, w] (reference raft_spline/utils.py:30-45 cvx_upsample, curves/base.py:35-38,
    95-123) with basis [T, d] on the device -> [B, T, n, 2] at the tile centres of the 8h x 8w image, one kernel forward and two
    backward (csrc/cvx_curves.hip) instead of the softmax / unfold / [B, 2d, 9, 8, 8, h, w] product / sum / permute chain.  The
    backward computes only the gradients autograd asks for: without a mask gradient the dense [B, 576, h, w] tensor is neither
    allocated nor filled.  No host synchronisation either way.  A basis matrix that requires grad (basis_grad='fused') gets its
    gradient behind those launches: the upsampled control points at the tile centres once more (mpc_pec_head_rows_dt, the mask
    read in its own dtype), then `_curve_basis_grad`."""

    @staticmethod
    def forward(ctx, params, up_mask, basis, scale: float, tile: int):
        _require_gpu(params, 'params')
        _require_gpu(up_mask, 'up_mask')
        B, c2, h, w = params.shape
        d, T, tile = c2 // 2, basis.shape[0], int(tile)
        dev = params.device
        p = _f32c(params.detach())
        m, m_dt = _net(up_mask)                       # (an fp16 / bf16 mask is read as it is: no .float() copy)
        bm = _f32c(basis.detach())
        s = tile // 2
        nty, ntx = ((v - s + tile - 1) // tile if v > s else 0 for v in (8 * h, 8 * w))          # (the count of the tile mask's centres)
        n = nty * ntx
        traj = torch.empty((B, T, n, 2), dtype=torch.float32, device=dev)
        if B * n > 0:                                 # (an empty tensor has no pointer to hand over: 8h or 8w within half a tile)
            _call('mpc_cvx_traj_fwd_dt', dev, _ptr(p), _ptr(m), m_dt, _ptr(bm), float(scale), _ptr(traj), B, d, T, h, w, tile, label='mpc_cvx_traj_fwd')
        ctx.save_for_backward(p, m, bm)
        ctx.dims = (B, d, T, h, w, tile, float(scale))
        return traj

    @staticmethod
    def backward(ctx, g):
        p, m, bm = ctx.saved_tensors
        B, d, T, h, w, tile, scale = ctx.dims
        g = _f32c(g)
        dev = g.device
        gp = gm = ws = None
        if g.numel() == 0:                            # no tile centre (or B = 0): no cotangent to hand over, and nothing reaches the inputs
            return (torch.zeros_like(p) if ctx.needs_input_grad[0] else None, torch.zeros_like(m) if ctx.needs_input_grad[1] else None,
                    torch.zeros_like(bm) if ctx.needs_input_grad[2] else None, None, None)
        if ctx.needs_input_grad[0]:
            gp = torch.empty((B, 2 * d, h, w), dtype=torch.float32, device=dev)
            ws = torch.empty(max(_query('mpc_cvx_traj_bwd_workspace_bytes', dev, B, d, T, h, w, tile), 4) // 4, dtype=torch.float32, device=dev)
        if ctx.needs_input_grad[1]:
            gm = torch.empty((B, 576, h, w), dtype=m.dtype, device=dev)                # (in the mask's dtype; every element is written by the kernel)
        if gp is not None or gm is not None:
            _call('mpc_cvx_traj_bwd_dt', dev, _ptr(g), _ptr(p), _ptr(m), _DT_CODE[m.dtype], _ptr(bm), scale, _ptr(gp), _ptr(gm), B, d, T, h, w, tile,
                  _ptr(ws), label='mpc_cvx_traj_bwd')
        gb = None
        if ctx.needs_input_grad[2]:
            n = g.shape[2]
            rows = torch.empty((B * n, 2 * d), dtype=torch.float32, device=dev)        # (scale 1: the reduction applies the node's scale once)
            _call('mpc_pec_head_rows_dt', dev, _ptr(p), _ptr(m), _DT_CODE[m.dtype], 1.0, tile, _ptr(rows), B, d, h, w, label='mpc_pec_head_rows')
            gb = _curve_basis_grad(g, rows, C.CBG_ROWS, scale, B, d, T, n)
        return gp, gm, gb, None, None


def cvx_flows(params, up_mask, basis, scale: float):
    """Dense flows of the upsampled curves [T, B, 2, 8h, 8w] ((x, y) order; reference: create_upsampled(mask).get_flow_from_reference
    (times) stacked): one kernel, forward only (csrc/cvx_curves.hip: mpc_cvx_flow_fwd)."""
    _require_gpu(params, 'params')
    _require_gpu(up_mask, 'up_mask')
    B, c2, h, w = params.shape
    d, T, dev = c2 // 2, basis.shape[0], params.device
    flows = torch.empty((T, B, 2, 8 * h, 8 * w), dtype=torch.float32, device=dev)
    p, (m, m_dt), bm = _f32c(params.detach()), _net(up_mask), _f32c(basis.detach())
    _call('mpc_cvx_flow_fwd_dt', dev, _ptr(p), _ptr(m), m_dt, _ptr(bm), float(scale), _ptr(flows), B, d, T, h, w, label='mpc_cvx_flow_fwd')
    return flows


def _corr_lookup_fwd(x, basis, lookup):
    """The forward launch of both lookup nodes -> (out, the detached x, d); basis None: x are coordinates, else Bezier control points."""
    _require_gpu(x, 'coords / params')
    dev = x.device
    bezier = basis is not None
    d = x.shape[1] // 2 if bezier else 0
    desc = lookup.descriptor(d)
    K = 2 * lookup.radius + 1
    out = torch.empty((lookup.B, lookup.num_entries * K * K, lookup.h, lookup.w), dtype=torch.float32, device=dev)
    xd = x.detach()
    _call('mpc_corr_lookup_fwd', dev, ctypes.byref(desc), None if bezier else _ptr(xd), _ptr(xd) if bezier else None, _ptr(basis), _ptr(out))
    return out, xd, d


def _corr_lookup_bwd(lookup, d, x, basis, g, want_x, grad_levels, flags=0):
    """The backward launch of both lookup nodes: the gradient of x (None unless `want_x`), and the level cotangents into the tensors of
    `grad_levels` (None: a level nobody asked for), written whole or, under MPC_CORR_F_GRAD_ACCUM in `flags`, added to."""
    return _corr_lookup_bwd_basis(lookup, d, x, basis, g, want_x, grad_levels, flags, False)[0]


def _corr_lookup_bwd_basis(lookup, d, x, basis, g, want_x, grad_levels, flags, want_basis):
    """`_corr_lookup_bwd` -> (the gradient of x, None unless `want_x`; the gradient of the basis matrix, None
    unless `want_basis`), and the level cotangents into the tensors of `grad_levels` (None: a level nobody asked for), written
    whole or, under MPC_CORR_F_GRAD_ACCUM in `flags`, added to.  `want_basis` (Bezier mode): the same launch also writes the targets'
    coordinate gradient [T, B, 2, h, w] -- alone, with grad_params NULL, where x is detached --, and `_curve_basis_grad` sums the
    matrix' gradient from it."""
    g = _f32c(g)
    desc = C.CorrDesc.from_buffer_copy(lookup.descriptor(d))
    desc.flags |= flags
    gx = torch.empty_like(x) if want_x else None
    for l, t in enumerate(grad_levels):
        desc.grad_level[l] = None if t is None else t.data_ptr()
    bez = basis is not None
    gc = torch.empty((basis.shape[0], lookup.B, 2, lookup.h, lookup.w), dtype=torch.float32, device=g.device) if bez and want_basis else None
    _call('mpc_corr_lookup_bwd', g.device, ctypes.byref(desc), None if bez else _ptr(x), _ptr(x) if bez else None, _ptr(basis), _ptr(g),
          _ptr(gc) if bez else _ptr(gx), _ptr(gx) if bez else None)
    gb = None if gc is None else _curve_basis_grad(gc, x, C.CBG_LOOKUP, 1.0, lookup.B, d, basis.shape[0], lookup.h * lookup.w)
    return gx, gb


class CorrLookupFn(torch.autograd.Function):
    """The RAFT-spline correlation lookup (utils.CorrLookup; reference corr.py:304-348, raft_spline/utils.py:4-20, raft.py:178-180):
    x = coords [T, B, 2, h, w] (basis None) or the Bezier control points params [B, 2d, h, w] with basis [T, d] on the device, and the
    pyramid levels of `lookup` as inputs of their own (so that autograd asks for their gradients) -> [B, E * (2r+1)^2, h, w], one
    kernel forward and one backward (csrc/corr_lookup.hip) instead of the coordinate tensor / grid_sample / cat / permute chain.
    The backward computes only what autograd asks for; every element of a gradient it returns is written by the kernel (no memset).
    A basis matrix that requires grad (a learned basis that trains, routed here by basis_grad='fused') gets its gradient too.
    The descriptor of the pyramid travels by value with the launch: no host synchronisation and no copy either way."""

    @staticmethod
    def forward(ctx, x, basis, lookup, *levels):
        out, xd, ctx.d = _corr_lookup_fwd(x, basis, lookup)
        ctx.lookup = lookup
        ctx.save_for_backward(xd, basis, *levels)
        return out

    @staticmethod
    def backward(ctx, g):
        x, basis, *levels = ctx.saved_tensors
        want_x, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_l = [ctx.needs_input_grad[3 + l] for l in range(len(levels))]
        if not want_x and not want_b and not any(want_l):
            return (None,) * (3 + len(levels))
        gl = [torch.empty_like(lv) if w else None for lv, w in zip(levels, want_l)]          # (every element is written by the kernel)
        gx, gb = _corr_lookup_bwd_basis(ctx.lookup, ctx.d, x, basis, g, want_x, gl, 0, want_b)
        return (gx, gb, None) + tuple(gl)


class CorrGradGate:
    """What the lookups of one `utils.CorrLookup(..., shared_grad=True)` share during a backward pass: `bufs`, one gradient buffer per
    level (None for a level that does not require grad), allocated and wholly written by the first lookup backward of the pass, added
    to by every later one, handed over and dropped by CorrGradGateFn.backward.  None between passes."""

    def __init__(self):
        self.bufs = None


class CorrGradGateFn(torch.autograd.Function):
    """The gate of `shared_grad=True`: the levels -> a one-element fp32 token that requires grad (nothing is copied, nothing is
    launched).  Every lookup of the object takes the token as its autograd input in the place of the levels
    (CorrLookupSharedFn), so this node's backward runs once, after the last lookup backward of the pass; it returns the shared buffers
    as the levels' gradients (None for a level that does not require grad, and for all of them when no lookup wrote any) and drops
    its references first: the next pass starts with a fresh whole fill.  No double backward."""

    @staticmethod
    def forward(ctx, gate, *levels):
        ctx.gate = gate
        ctx.set_materialize_grads(False)                              # (the lookups return no gradient for the token: None arrives)
        return torch.empty(1, dtype=torch.float32, device=levels[0].device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        bufs, ctx.gate.bufs = ctx.gate.bufs, None
        n = len(ctx.needs_input_grad) - 1
        if bufs is None:
            return (None,) * (1 + n)
        return (None,) + tuple(b if ctx.needs_input_grad[1 + l] else None for l, b in enumerate(bufs))


class CorrLookupSharedFn(torch.autograd.Function):
    """CorrLookupFn under `shared_grad=True`: the same kernels over the same level storage (`lookup.levels`), with the gate's token as the
    autograd input in the place of the levels.  The backward writes grad_coords / grad_params as CorrLookupFn does.  When the engine is
    going to run the gate's node in this pass (some level's gradient was asked for), the level cotangents go into the gate's buffers:
    the first lookup backward of the pass allocates them (torch.empty_like) and runs the whole-slice fill, every later one runs
    MPC_CORR_F_GRAD_ACCUM, which adds its window cells and touches nothing else.  The token gets no gradient (None): the edge alone keeps
    the gate's backward after every lookup's.  One launch per backward, no host synchronisation, capturable on one stream."""

    @staticmethod
    def forward(ctx, x, basis, lookup, token):
        out, xd, ctx.d = _corr_lookup_fwd(x, basis, lookup)
        ctx.lookup, ctx.gate_node = lookup, token.grad_fn
        ctx.save_for_backward(xd, basis)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, basis = ctx.saved_tensors
        lookup, gate = ctx.lookup, ctx.lookup._gate
        want_x, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # needs_input_grad is fixed at the forward; whether THIS pass reaches the levels is the engine's to say
        want_l = ctx.needs_input_grad[3] and ctx.gate_node is not None and torch._C._will_engine_execute_node(ctx.gate_node)
        if not want_x and not want_b and not want_l:
            return None, None, None, None
        flags = 0
        if want_l:
            if gate.bufs is None:                                     # the first of the pass: every element is written by the kernel
                gate.bufs = [torch.empty_like(lv) if lv.requires_grad else None for lv in lookup.levels]
            else:
                flags = C.CORR_F_GRAD_ACCUM
        gx, gb = _corr_lookup_bwd_basis(lookup, ctx.d, x, basis, g, want_x, gate.bufs if want_l else (), flags, want_b)
        return gx, gb, None, None


def corr_pyramid_desc(B, h, w, num_levels_per_target):
    """The C descriptor (include/mpcmax.h: mpc_corr_desc) of a pyramid over a [B, ., h, w] grid, without level pointers."""
    nl = [int(v) for v in num_levels_per_target]
    tix = [[t for t, v in enumerate(nl) if v >= l + 1] for l in range(max(nl))]
    desc = C.CorrDesc(B=int(B), h=int(h), w=int(w), T=len(nl), d=0, radius=1, num_levels=len(tix))
    for l, ts in enumerate(tix[:C.CORR_MAX_LEVELS]):
        desc.level_h[l], desc.level_w[l], desc.level_n[l] = h >> l, w >> l, len(ts)
        for s, t in enumerate(ts[:C.CORR_MAX_TARGETS]):
            desc.level_target[l][s] = t
    return desc, tix


def _corr_pyramid_ws(desc, D, backward, dev):
    nws = _query('mpc_corr_pyramid_workspace_bytes', dev, ctypes.byref(desc), D, backward)
    return torch.empty((nws + 3) // 4, dtype=torch.float32, device=dev)


class CorrPyramidFn(torch.autograd.Function):
    """The RAFT-spline correlation pyramid (utils.corr_pyramid_fused; reference corr.py:235-270, 106-123): fmap1 [B, D, h, w],
    fmap2 [T, B, D, h, w] (both fp32, both fp16 or both bf16; contiguous, on the GPU) and the host list of level counts -> the levels
    [n_l, B*h*w, 1, h_l, w_l], fp32 whatever the maps are, as a tuple, one autograd node (csrc/corr_pyramid.hip: every level is its
    own fp32-MFMA GEMM against the pooled feature map, written once).  16-bit maps are read in place (no .float() copy): level 0 runs
    on the 16-bit matrix cores -- the same sum in another order --, everything else is the fp32 arithmetic on the upcast maps bit
    for bit, and the gradients come back in the maps' dtype, rounded once.  The backward computes only the requested gradients, takes
    a missing level cotangent as zero, and every element of a gradient it returns is written by a kernel (no memset).  No host
    synchronisation; bitwise reproducible."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels_per_target):
        _require_gpu(fmap1, 'fmap1')
        _require_gpu(fmap2, 'fmap2')
        T, B, D, h, w = fmap2.shape
        dev = fmap1.device
        desc, tix = corr_pyramid_desc(B, h, w, num_levels_per_target)
        levels = [torch.empty((len(ts), B * h * w, 1, h >> l, w >> l), dtype=torch.float32, device=dev) for l, ts in enumerate(tix)]
        (f1, dt), (f2, dt2) = _net(fmap1), _net(fmap2)
        if dt != dt2:
            raise ValueError(f'CorrPyramidFn: fmap1 is {fmap1.dtype}, fmap2 {fmap2.dtype}: one dtype per call')
        if B > 0:
            for l, lv in enumerate(levels):
                desc.level[l] = lv.data_ptr()
            ws = _corr_pyramid_ws(desc, D, 0, dev)
            _call('mpc_corr_pyramid_fwd_dt', dev, ctypes.byref(desc), D, _ptr(f1), _ptr(f2), dt, _ptr(ws), label='mpc_corr_pyramid_fwd')
        ctx.nl = [int(v) for v in num_levels_per_target]
        ctx.set_materialize_grads(False)                              # (an unused level arrives as None, not as a volume of zeros)
        ctx.save_for_backward(f1, f2)
        return tuple(levels)

    @staticmethod
    def backward(ctx, *gl):
        f1, f2 = ctx.saved_tensors
        T, B, D, h, w = f2.shape
        dev = f1.device
        want1, want2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not want1 and not want2:
            return None, None, None
        g1 = torch.empty_like(f1) if want1 else None                  # (every element is written by a kernel; in the maps' dtype)
        g2 = torch.empty_like(f2) if want2 else None
        if B > 0:
            desc, _ = corr_pyramid_desc(B, h, w, ctx.nl)
            gl = [None if g is None else _f32c(g) for g in gl]
            for l, g in enumerate(gl):
                desc.grad_level[l] = None if g is None else g.data_ptr()
            ws = _corr_pyramid_ws(desc, D, 1, dev)
            _call('mpc_corr_pyramid_bwd_dt', dev, ctypes.byref(desc), D, _ptr(f1), _ptr(f2), _ptr(g1), _ptr(g2), _DT_CODE[f1.dtype], _ptr(ws),
                  label='mpc_corr_pyramid_bwd')
        return g1, g2, None


def corr_pyramid_refs(counts):
    """The C descriptor (include/mpcmax.h: mpc_corr_refs) of references with `counts` targets each, without tensor pointers."""
    refs = C.CorrRefs(R=len(counts))
    for r, n in enumerate(counts[:C.CORR_MAX_REFS]):
        refs.first_target[r + 1] = refs.first_target[r] + int(n)
    return refs


class CorrPyramidMultiFn(torch.autograd.Function):
    """CorrPyramidFn over several references (utils.corr_pyramid_fused in list form; reference corr.py:221-225, 246-260, 282-302:
    the events-plus-frames pyramid): `num_levels` the host list of R lists of level counts, then fmap1[0..R) [B, D, h, w] and
    fmap2[0..R) [n_r, B, D, h, w] (all fp32, all fp16 or all bf16 -- as CorrPyramidFn --, contiguous, on one GPU) -> the fp32
    levels of the merged target list as a tuple, one autograd
    node with the launches of the single-reference node (csrc/corr_pyramid.hip: a slot reads the feature maps of its reference where
    they lie).  The backward computes only the requested ones of the 2R gradients, each written straight into its own tensor, every
    element by a kernel; a missing level cotangent is zero.  Equal, bit for bit, to the R single-reference nodes."""

    @staticmethod
    def forward(ctx, num_levels, *fmaps):
        R = len(fmaps) // 2
        for i, t in enumerate(fmaps):
            _require_gpu(t, f'fmap{1 + i // R}[{i % R}]')
        B, D, h, w = fmaps[0].shape
        dev = fmaps[0].device
        nl = [int(v) for ref in num_levels for v in ref]
        desc, tix = corr_pyramid_desc(B, h, w, nl)
        levels = [torch.empty((len(ts), B * h * w, 1, h >> l, w >> l), dtype=torch.float32, device=dev) for l, ts in enumerate(tix)]
        fm = [_net(t)[0] for t in fmaps]
        if len({t.dtype for t in fm}) != 1:
            raise ValueError(f'CorrPyramidMultiFn: feature maps of dtypes {[str(t.dtype) for t in fmaps]}: one dtype per call')
        if B > 0:
            for l, lv in enumerate(levels):
                desc.level[l] = lv.data_ptr()
            refs = corr_pyramid_refs([len(ref) for ref in num_levels])
            for r in range(R):
                refs.fmap1[r], refs.fmap2[r] = fm[r].data_ptr(), fm[R + r].data_ptr()
            nws = _query('mpc_corr_pyramid_multi_workspace_bytes', dev, ctypes.byref(desc), D, ctypes.byref(refs), 0)
            ws = torch.empty((nws + 3) // 4, dtype=torch.float32, device=dev)
            _call('mpc_corr_pyramid_multi_fwd_dt', dev, ctypes.byref(desc), D, ctypes.byref(refs), _DT_CODE[fm[0].dtype], _ptr(ws),
                  label='mpc_corr_pyramid_multi_fwd')
        ctx.num_levels = [[int(v) for v in ref] for ref in num_levels]
        ctx.set_materialize_grads(False)                              # (an unused level arrives as None, not as a volume of zeros)
        ctx.save_for_backward(*fm)
        return tuple(levels)

    @staticmethod
    def backward(ctx, *gl):
        fm = ctx.saved_tensors
        R = len(fm) // 2
        B, D, h, w = fm[0].shape
        dev = fm[0].device
        want = ctx.needs_input_grad[1:]
        if not any(want):
            return (None,) * (1 + 2 * R)
        grads = [torch.empty_like(t) if wanted else None for t, wanted in zip(fm, want)]          # (every element is written by a kernel)
        if B > 0:
            desc, _ = corr_pyramid_desc(B, h, w, [v for ref in ctx.num_levels for v in ref])
            gl = [None if g is None else _f32c(g) for g in gl]
            for l, g in enumerate(gl):
                desc.grad_level[l] = None if g is None else g.data_ptr()
            refs = corr_pyramid_refs([len(ref) for ref in ctx.num_levels])
            for r in range(R):
                refs.fmap1[r], refs.fmap2[r] = fm[r].data_ptr(), fm[R + r].data_ptr()
                refs.grad_fmap1[r] = None if grads[r] is None else grads[r].data_ptr()
                refs.grad_fmap2[r] = None if grads[R + r] is None else grads[R + r].data_ptr()
            nws = _query('mpc_corr_pyramid_multi_workspace_bytes', dev, ctypes.byref(desc), D, ctypes.byref(refs), 1)
            ws = torch.empty((nws + 3) // 4, dtype=torch.float32, device=dev)
            _call('mpc_corr_pyramid_multi_bwd_dt', dev, ctypes.byref(desc), D, ctypes.byref(refs), _DT_CODE[fm[0].dtype], _ptr(ws),
                  label='mpc_corr_pyramid_multi_bwd')
        return (None, *grads)


class GridTrajFn(torch.autograd.Function):
    """The network's coefficient grid [B, S, 2k, H, W] -> `trajectories` [B, n_t, n, 2] (y, x) at the tile centres (row A3 of SURVEY.md
    8(a): reference trajectory_net.py:57-119): one kernel forward, one backward (two when `dphi` needs a gradient), csrc/grid_traj.hip,
    instead of the mask gather / compute_basis / permute chain of plain torch and its adjoints.  basis: C.BASIS_POLY or C.BASIS_DCT
    (evaluated by the kernels from the device `times`: `dphi` is None) or C.BASIS_MATRIX (`dphi` [n_t, k] = net(times) - net(anchor),
    differentiable).  No host synchronisation either way; `times` gets no gradient (the reference does not differentiate them)."""

    @staticmethod
    def forward(ctx, coeff_grid, times, dphi, basis: int, anchor: float, add_offsets: bool, tile: int):
        _require_gpu(coeff_grid, 'coeff_grid')
        B, S, c2, H, W = coeff_grid.shape
        k, dev = c2 // 2, coeff_grid.device
        cg, cg_dt = _net(coeff_grid)                  # (fp16 / bf16 grids are read as they are: no .float() copy)
        tm = None if times is None else _f32c(times.detach()).reshape(-1)
        dp = None if dphi is None else _f32c(dphi.detach())
        n_t = dp.shape[0] if dp is not None else tm.shape[0]
        s = tile // 2
        hq = (H - s + tile - 1) // tile if H > s else 0
        wq = (W - s + tile - 1) // tile if W > s else 0
        traj = torch.empty((B, n_t, hq * wq, 2), dtype=torch.float32, device=dev)
        rows = None
        if dp is not None and ctx.needs_input_grad[2]:        # (saved only when the basis itself is learned)
            rows = torch.empty((B * hq * wq, c2), dtype=torch.float32, device=dev)
        _call('mpc_grid_traj_fwd_dt', dev, _ptr(cg), cg_dt, _ptr(tm), _ptr(dp), int(basis), float(anchor), int(bool(add_offsets)), _ptr(traj),
              _ptr(rows), B, S, k, H, W, int(tile), n_t, label='mpc_grid_traj_fwd')
        ctx.save_for_backward(tm, dp, rows)
        ctx.dims = (B, S, k, H, W, int(tile), n_t, int(basis), float(anchor))
        ctx.grid_dtype = cg.dtype
        return traj

    @staticmethod
    def backward(ctx, g):
        tm, dp, rows = ctx.saved_tensors
        B, S, k, H, W, tile, n_t, basis, anchor = ctx.dims
        g = _f32c(g)
        dev = g.device
        gg = torch.empty((B, S, 2 * k, H, W), dtype=ctx.grid_dtype, device=dev)         # (in the grid's dtype; every element is written by the kernel)
        gd = scratch = None
        if rows is not None:
            nsc = _query('mpc_grid_traj_scratch_floats', dev, B, k, H, W, tile, n_t)
            gd = torch.empty((n_t, k), dtype=torch.float32, device=dev)
            scratch = torch.empty(max(nsc, 1), dtype=torch.float32, device=dev)
        _call('mpc_grid_traj_bwd_dt', dev, _ptr(g), _ptr(tm), _ptr(dp), basis, anchor, _ptr(rows), _ptr(gg), _DT_CODE[ctx.grid_dtype], _ptr(gd),
              _ptr(scratch), B, S, k, H, W, tile, n_t, label='mpc_grid_traj_bwd')
        return gg, None, gd, None, None, None, None


def knn_indices(cfg: PathConfig, trajectories):
    """Debug/test helper: the K neighbour indices [B, nb, Q, K] (ascending distance, index)."""
    _require_gpu(trajectories, 'trajectories')
    traj = _f32c(trajectories.detach())
    B, _, n, _ = traj.shape
    shape = make_shape(cfg, B, 0, 0, n)
    if knn_is_wide(n):
        return knn_wide_fwd(cfg, shape, traj)[2]
    ws = alloc_workspace(shape, traj.device)
    _, _, _, idx = knn_lut_fwd(cfg, shape, traj, ws, want_idx=True)
    return idx


def splat_events(image_shape, pos_weight_rows, unit_weight, blur):
    """imager path (reference event_image_converter.py:45-74,134-176 'bilinear_vote'):
    rows [nimg, m, 6] with (y, x, -, -, -, weight) -> [nimg, H, W], optionally blurred."""
    _require_gpu(pos_weight_rows, 'events')
    rows = _f32c(pos_weight_rows)
    nimg, m, _ = rows.shape
    cfg = PathConfig(image_shape=tuple(image_shape), num_tref=1, num_bins=1, num_knn=0, smooth_weight=0.0,
                     sp=max(image_shape), norm_l2=False, dist_l1=False, scale_by_dt=False, mask_border=False,
                     polarity_split=False, scheme_iwd=False, smooth_on_next=False)
    extra = C.F_NO_WARP | (C.F_UNIT_WEIGHT if unit_weight else 0)
    shape = make_shape(cfg, nimg, m, m, 0, extra_flags=extra, K=0)
    ws = alloc_workspace(shape, rows.device)
    raw = event_splat_fwd(shape, rows, None, None, ws)
    if blur:
        raw, _ = contrast_fwd(shape, raw, ws, False)
    return raw[:, 0]
