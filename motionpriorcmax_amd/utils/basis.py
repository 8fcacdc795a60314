"""Motion bases evaluated at the reconstruction times (host side, plain torch: 1 + num_bins
times x ~19k trajectories).  Mirrors reference src/utils/basis.py:4-46 and the Bernstein basis of
src/models/raft_spline/curves/bezier.py:69-107."""
import math
import weakref

import numpy as np
import torch


def compute_basis(coeffs, times, num_basis, basis_type, basis_network=None):
    """coeffs [b, s, 2, n, k], times [n_t] -> trajectories [b, n, n_t, 2] summed over scales s."""
    if basis_type == "dct":
        k_idx = torch.arange(1, num_basis + 1, device=coeffs.device)
        basis = np.sqrt(2.0) * torch.cos(np.pi / 2.0 * ((2 * times[..., None] + 1) * k_idx[None, None, :]))
    elif basis_type == "learned":
        basis = basis_network(times[..., None])
    elif basis_type == "polynomial":
        k_idx = torch.arange(1, num_basis + 1, device=coeffs.device)
        basis = times[..., None] ** k_idx[None, None, :]
    else:
        raise ValueError
    cy = coeffs[..., 0, :, :]
    cx = coeffs[..., 1, :, :]
    ty = torch.sum(basis[..., None, :, :] * cy[..., None, :], dim=-1)
    tx = torch.sum(basis[..., None, :, :] * cx[..., None, :], dim=-1)
    return torch.sum(torch.stack([ty, tx], dim=-1), dim=1)


def basis_values(times, num_basis, basis_type, basis_network=None):
    """The basis functions of `compute_basis` at arbitrary times: times [...] -> [..., k] (same formulas, same dtype as `times`).
    Used by the per-event continuous-time warp (FocusLoss.calc_per_event_basis: UNPINNED extension), which evaluates the basis at
    every event's own timestamp instead of at the num_bins bin mid-times."""
    if basis_type == "dct":
        k_idx = torch.arange(1, num_basis + 1, device=times.device)
        return np.sqrt(2.0) * torch.cos(np.pi / 2.0 * ((2 * times[..., None] + 1) * k_idx))
    if basis_type == "learned":
        return basis_network(times[..., None])
    if basis_type == "polynomial":
        k_idx = torch.arange(1, num_basis + 1, device=times.device)
        return times[..., None] ** k_idx
    raise ValueError(basis_type)


def table_basis_values(table, times):
    """A TABULATED basis at arbitrary times: table [S + 1, k] holds samples of the k basis functions at the knots i / S, times [...]
    -> [..., k], interpolated linearly.  This is the definition of FocusLoss.calc_per_event_basis(basis_type='table') and the lines
    are those of the kernels (csrc/pe_device.h: pe_tab_locate; csrc/pe_basis.hip: pe_tab_basis), one operation each, so that the fp32 result agrees
    with them bit for bit: times outside [0, 1] are clamped, t == 1 lies in the last interval with f == 1.  Plain torch, any floating
    dtype (the promotion of the two arguments'), differentiable w.r.t. `table`."""
    if table.dim() != 2 or table.shape[0] < 2:
        raise ValueError(f'basis table must be [samples + 1, k] with samples >= 1, got {tuple(table.shape)}')
    S = table.shape[0] - 1
    dtype = torch.promote_types(table.dtype, times.dtype)
    table, times = table.to(dtype), times.to(dtype)
    tc = times.clamp(min=0).clamp(max=1)
    x = tc * float(S)
    i = x.floor().to(torch.int64).clamp(max=S - 1)
    f = x - i.to(dtype)
    lo = table[i]
    return lo + f[..., None] * (table[i + 1] - lo)


CURVE_EVENT_TYPES = ('BEZIER', 'POLYNOMIAL', 'TABLE', 'BSPLINE')
BSPLINE_MIN_DEGREE = 3


def _bspline_event_basis(t, d):
    """'BSPLINE' of `curve_event_basis`, its lines one by one (t fp32 [...] -> [..., d])."""
    L = d - 2
    tc = t.clamp(min=0).clamp(max=1)
    x = tc * float(L)
    s = x.floor().to(torch.int64).clamp(min=0, max=L - 1)
    u = {k: (s + k).clamp(min=0, max=L).to(torch.float32) for k in range(-2, 4)}       # scaled knots: exact small integers
    N = [torch.ones_like(x), None, None, None]
    for j in range(1, 4):
        saved = torch.zeros_like(x)
        for r in range(j):
            right, left, den = u[r + 1] - x, x - u[1 - j + r], u[r + 1] - u[1 - j + r]
            temp = N[r] / den                   # (tensor / tensor: a division, correctly rounded; never by a Python scalar)
            N[r] = saved + right * temp
            saved = left * temp
        N[j] = saved
    # E_{s-1+q} = N_q: scattered into the d + 1 functions of the spline (s + q <= L + 2 = d), then function 0 (P0 = 0) is dropped
    E = torch.zeros(t.shape + (d + 1,), dtype=torch.float32, device=t.device)
    E.scatter_(-1, torch.stack([s + q for q in range(4)], dim=-1), torch.stack(N, dim=-1))
    return E[..., 1:]


def curve_event_basis(times, d, curve_type, basis_table=None):
    """The basis E of FocusLoss.calc_per_event_curves at arbitrary times: times [...] -> [..., d] in fp32, on the device of `times`,
    nothing read back.  This is the DEFINITION and the lines are those of the kernels (csrc/pe_curves.hip: pec_basis), one fp32
    operation each, so that the two agree bit for bit:
      'BEZIER'      u = 1 - t;  tp_1 = t, tp_i = tp_{i-1} * t;  up_0 = 1, up_1 = u, up_i = up_{i-1} * u;
                    E_i = (C(d, i) * tp_i) * up_{d-i}, i = 1..d (P0 = 0: reference curves/bezier.py:92-113).  At t = 0 every E_i is
                    exactly 0; at t = 1, E_d is exactly 1 and the others exactly 0 (the shortcut rows of curves/base.py:102-106).
                    The binomials are exact fp32 constants up to d = 26 (the kernels serve d <= 16).
      'POLYNOMIAL'  E_1 = t, E_i = E_{i-1} * t (the lines of pe_phi, csrc/pe_basis.hip; curves/polynomial.py:55-58 up to the rounding
                    of pow)
      'TABLE'       `table_basis_values(basis_table, t)`: basis_table [S + 1, d] sampled at the knots i / S, interpolated linearly
                    (a frozen learned basis, say; the cubic B-spline has a kind of its own)
      'BSPLINE'     the clamped (open-uniform) cubic B-spline of `bspline_basis` with d + 1 control points (P0 = 0), L = d - 2 spans,
                    d >= 3, exactly -- no table:
                      tc = min(max(t, 0), 1);  x = tc * (float)L;  s = min((int)floorf(x), L - 1)
                      u(k) = (float)min(max(s + k, 0), L)          scaled knots, exact small integers, k = -2..3
                      N_0 = 1
                      for j = 1..3:  saved = 0
                          for r = 0..j-1:
                              right = u(r+1) - x;   left = x - u(1-j+r);   den = u(r+1) - u(1-j+r)      (den is 1, 2 or 3, never 0)
                              temp = N_r / den;     N_r = saved + right * temp;     saved = left * temp
                          N_j = saved
                      E_{s-1+q} = N_q, q = 0..3   (index -1 is P0 and is dropped);   every other E_j = +0
                    (The NURBS Book's BasisFuns on the knots scaled by L; the division is correctly rounded.)  At t = 0 every E_j is
                    exactly 0, at t = 1 E_d is exactly 1 and the others exactly 0; at most 4 of the d are non-zero; d = 3 is the cubic
                    Bezier curve."""
    d = int(d)
    if d < 1:
        raise ValueError(f'degree must be >= 1, got {d}')
    if curve_type not in CURVE_EVENT_TYPES:
        raise ValueError(f'curve_type must be one of {CURVE_EVENT_TYPES}, got {curve_type!r}')
    if (curve_type == 'TABLE') != (basis_table is not None):
        raise ValueError("curve_type='TABLE' and basis_table go together")
    t = times.to(torch.float32)
    if curve_type == 'BSPLINE':
        if d < BSPLINE_MIN_DEGREE:
            raise ValueError(f"curve_type='BSPLINE' is cubic: it needs d >= {BSPLINE_MIN_DEGREE} control points per axis beside P0, got {d}")
        return _bspline_event_basis(t, d)
    if curve_type == 'TABLE':
        if basis_table.dim() != 2 or basis_table.shape[1] != d or basis_table.dtype != torch.float32:
            raise ValueError(f'basis_table must be float32 [samples + 1, {d}], got {tuple(basis_table.shape)} {basis_table.dtype}')
        return table_basis_values(basis_table.detach().to(t.device), t)
    if curve_type == 'POLYNOMIAL':
        cols = [t]
        for _ in range(1, d):
            cols.append(cols[-1] * t)
        return torch.stack(cols, dim=-1)
    u = 1 - t
    tp = [t]                                   # tp[i - 1] = t^i
    for _ in range(1, d):
        tp.append(tp[-1] * t)
    up = [torch.ones_like(t), u]               # up[i] = u^i
    for _ in range(2, d):
        up.append(up[-1] * u)
    return torch.stack([(float(math.comb(d, i)) * tp[i - 1]) * up[d - i] for i in range(1, d + 1)], dim=-1)


def curve_head_rows(params, up_mask, scale, tile):
    """The tile rows of FocusLoss.calc_per_event_curves in plain torch (the mirror of mpc_pec_head_rows): params [B, 2d, h, w] (x
    channels first) -> [B * G, 2d] with rows[(b, cell)][j] = scale * up_y[j], rows[(b, cell)][d + j] = scale * up_x[j], `up` the
    convex upsampling (`_cvx_upsample`) read at the tile centres (iy * tile + tile // 2, ix * tile + tile // 2) of the 8h x 8w
    image, or `params` themselves without a mask (h x w is the tile grid then).  The tile centre is never added.  Differentiable."""
    B, c2, h, w = params.shape
    d = c2 // 2
    if up_mask is not None:
        up = _cvx_upsample(params, up_mask)[:, :, tile // 2::tile, tile // 2::tile]
    else:
        up = params
    up = float(scale) * up
    G = up.shape[2] * up.shape[3]
    return torch.cat((up[:, d:], up[:, :d]), dim=1).reshape(B, c2, G).permute(0, 2, 1).reshape(B * G, c2)


def basis_table(basis_type, num_basis, samples, basis_network=None, device=None):
    """The table of `table_basis_values` for one of the bases of `basis_values`: its values at the samples + 1 knots i / samples,
    [samples + 1, num_basis] fp32, plain torch and differentiable through `basis_network`.  Training the reference's learned basis
    through the per-event warp is `T = basis_table('learned', k, 1024, net)` once per step: the network runs at 1025 knots
    instead of at every event, and autograd carries the table's gradient into its weights."""
    samples = int(samples)
    if samples < 1:
        raise ValueError('samples must be >= 1')
    if device is None and basis_network is not None:
        device = next((p.device for p in basis_network.parameters()), None)
    knots = torch.arange(samples + 1, dtype=torch.float32, device=device) / float(samples)
    return basis_values(knots, num_basis, basis_type, basis_network)


_BASIS_CACHE = {}


def _cached_basis(kind, times, *args):
    """The [n_t, d] basis matrix of `kind` for these timestamps: the float64 evaluation runs on the host (as the reference's does,
    bezier.py:104-107) and costs milliseconds -- a training loop asks for the same bin mid-times every step, so the last few
    matrices are kept (keyed on the timestamps' bytes)."""
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
    key = (kind, args, t.tobytes())
    m = _BASIS_CACHE.get(key)
    if m is None:
        if len(_BASIS_CACHE) > 32:
            _BASIS_CACHE.clear()
        m = _BASIS_CACHE[key] = _BASIS_EVAL[kind](t, *args)
    return m


_DEV_BASIS_CACHE = []          # [(times tensor, its version, kind, args, device, dtype, matrix on the device)]
_TILE_POS_CACHE = {}


def _device_basis(kind, times, args, device, dtype):
    """The basis matrix on `device`.  A training loop passes the SAME timestamps tensor every step: for a tensor seen before (the
    object itself, unmodified -- the entry holds a reference, so its address cannot be handed to another tensor) the matrix is
    returned without reading the timestamps back to the host (a device synchronisation, the float64 evaluation and an upload: 9 ms
    of a 0.3 ms step)."""
    if torch.is_tensor(times):
        # an entry belongs to a tensor OBJECT (weak reference: the cache keeps no caller tensor alive; a dead entry cannot match, so
        # an address handed to another tensor is no hit), unmodified as far as torch can tell (_version) and still at the same
        # storage address with the same shape (`.data` assignments and set_() do not bump the version)
        _DEV_BASIS_CACHE[:] = [e for e in _DEV_BASIS_CACHE if e[0]() is not None]
        for ent in _DEV_BASIS_CACHE:
            if ent[0]() is times and ent[1] == (times._version, times.data_ptr(), tuple(times.shape)) and ent[2:6] == (kind, args, device, dtype):
                return ent[6]
        t = times.detach().cpu().numpy()
    else:
        t = times
    m = _cached_basis(kind, t, *args).to(device, dtype)
    if torch.is_tensor(times):
        if len(_DEV_BASIS_CACHE) >= 8:
            _DEV_BASIS_CACHE.pop(0)
        _DEV_BASIS_CACHE.append((weakref.ref(times), (times._version, times.data_ptr(), tuple(times.shape)), kind, args, device, dtype, m))
    return m


def _tile_positions(H, W, tile_size, device, dtype):
    """(tile centres as a LongTensor on the host -- what the adapters return --, the same on `device` in `dtype`), built once.
    The adapters hand the host tensor out as it is (a copy per step would be host time of a host-bound step): their docstrings say
    that `pixel_positions` is shared and must not be modified in place."""
    from .trajectories import get_optical_flow_tile_mask
    key = (H, W, tile_size, str(device), dtype)
    ent = _TILE_POS_CACHE.get(key)
    if ent is None:
        if len(_TILE_POS_CACHE) > 16:
            _TILE_POS_CACHE.clear()
        pos = torch.nonzero(get_optical_flow_tile_mask((H, W), tile_size))
        ent = _TILE_POS_CACHE[key] = (pos, pos.to(device, dtype))
    return ent


def _basis_dtype(params):
    """The dtype of the basis matrix of the curve adapters: that of `params`, except fp32 for fp16 / bf16 control points on the GPU
    -- those run in the fused nodes, which evaluate in fp32 (a Bernstein matrix rounded to bf16 would cost the curve 8 of its 24
    bits for nothing); where such a tensor still takes a plain-torch mirror (a shape beyond the kernels' limits), the mirror rounds
    the matrix to the dtype of `params`, as it always did."""
    return torch.float32 if params.is_cuda and params.dtype in (torch.float16, torch.bfloat16) else params.dtype


def _basis_trains(bm):
    """Does autograd want the gradient of this basis matrix (the reference's curve_type LEARNED while its basis network trains)?  The
    fused nodes treat the matrix as a constant (ops.CurveTrajFn, ops.CvxCurveTrajFn, ops.CorrLookupFn return None for it), so such a
    matrix takes the plain-torch mirrors, where it is an ordinary autograd input."""
    return torch.is_grad_enabled() and bm.requires_grad


BASIS_GRAD_ROUTES = ('mirror', 'fused')


def _basis_grad_fused(basis_grad):
    """The keyword `basis_grad` of `trajectories_from_curves` / `CorrLookup.lookup_curves` checked -> is it 'fused'."""
    if basis_grad not in BASIS_GRAD_ROUTES:
        raise ValueError(f'basis_grad must be one of {BASIS_GRAD_ROUTES}, got {basis_grad!r}')
    return basis_grad == 'fused'


def _basis_served(bm, fused):
    """May the fused nodes take this basis matrix: a constant to autograd, or -- basis_grad='fused' -- one that trains and lies within
    the limit of its gradient's reduction (mpc_curve_basis_grad: the nodes' own 48 KB)."""
    return not _basis_trains(bm) or (fused and bm.shape[0] * bm.shape[1] * 4 <= 48 * 1024)


def _curve_trajectories(params, bm, tile_size, H, W, scale, fused=False):
    """pos + scale * (basis x control points), (y, x) order: on the GPU one kernel each way (ops.CurveTrajFn, csrc/curves.hip:
    mpc_curve_traj_fwd / _bwd -- a training step calls this every iteration and a B = 1 step is bound by the host); for CPU tensors
    (the host-side tests against the reference's curves) the same in plain torch.  `fused`: a basis matrix that requires grad
    takes the node too, which then returns its gradient (csrc/curve_basis.hip)."""
    B, c2, h, w = params.shape
    d = c2 // 2
    if params.is_cuda and params.dtype in _KERNEL_DTYPES and d <= 16 and _basis_served(bm, fused):
        # (fp16 / bf16 control points go through a differentiable .float() -- autograd casts their gradient back --, and the basis
        # matrix and the tile positions are fp32 whatever params.dtype is: the trajectories are fp32, never positions in 16 bits)
        from .. import ops
        pos, pos_dev = _tile_positions(H, W, tile_size, params.device, torch.float32)
        assert pos.shape[0] == h * w, 'image shape must be a multiple of the tile size'
        return ops.CurveTrajFn.apply(params.float(), bm.float(), pos_dev, float(scale)), pos
    pos, pos_dev = _tile_positions(H, W, tile_size, params.device, params.dtype)
    assert pos.shape[0] == h * w, 'image shape must be a multiple of the tile size'
    flow = torch.einsum('bcdhw,td->btchw', params.view(B, 2, d, h, w), bm.to(params.dtype)) * scale  # [B, n_t, (x, y), h, w]
    disp = torch.stack((flow[:, :, 1], flow[:, :, 0]), dim=-1).reshape(B, bm.shape[0], h * w, 2)
    return disp + pos_dev[None, None], pos


def _cvx_upsample(params, up_mask):
    """The convex upsampling of reference src/models/raft_spline/utils.py:30-45 written from its formula (a softmax over the nine
    neighbours, a zero pad, nine shifted multiply-adds in F.unfold's row-major order, the factor 8 inside):
    params [B, C, h, w], up_mask [B, 576, h, w] (channel = k * 64 + sy * 8 + sx) -> [B, C, 8h, 8w]."""
    B, C, h, w = params.shape
    wts = torch.softmax(up_mask.reshape(B, 9, 8, 8, h, w), dim=1)
    p8 = torch.nn.functional.pad(8 * params, (1, 1, 1, 1))
    up = None
    for k in range(9):
        dy, dx = k // 3, k % 3
        term = wts[:, None, k] * p8[:, :, None, None, dy:dy + h, dx:dx + w]            # [B, C, 8, 8, h, w]
        up = term if up is None else up + term
    return up.permute(0, 1, 4, 2, 5, 3).reshape(B, C, 8 * h, 8 * w)


_CVX_KERNEL_TILES = (2, 4, 8, 16)
_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)          # what the fused nodes take (the mask in place: include/mpcmax.h, MPC_DT_*)


def _cvx_kernels_serve(params, up_mask, bm, fused=False):
    """The routing rule of `_curve_trajectories`: the kernels take fp32, fp16 or bf16 GPU tensors (the mask is read in its own dtype,
    the control points go through .float()) with d <= 16 and a basis matrix within their 48 KB LDS slice that is a constant to
    autograd; everything else (CPU tensors, other dtypes, d > 16, more times, a basis matrix that requires grad) runs in plain
    torch.  `fused` (basis_grad='fused'): a basis matrix that requires grad is served too."""
    return (params.is_cuda and up_mask.is_cuda and params.dtype in _KERNEL_DTYPES and up_mask.dtype in _KERNEL_DTYPES
            and params.shape[1] // 2 <= 16 and bm.shape[0] * bm.shape[1] * 4 <= 48 * 1024 and _basis_served(bm, fused))


def _cvx_curve_trajectories_mirror(params, up_mask, bm, pos_dev, scale):
    """Plain torch: the upsampled control points at the tile centres, then the curve product of `_curve_trajectories`."""
    B, c2, h, w = params.shape
    d = c2 // 2
    idx = pos_dev.long()
    up = _cvx_upsample(params, up_mask)[:, :, idx[:, 0], idx[:, 1]]                     # [B, 2d, n]
    flow = torch.einsum('bcdn,td->btcn', up.reshape(B, 2, d, -1), bm.to(up.dtype)) * scale           # [B, n_t, (x, y), n]
    disp = torch.stack((flow[:, :, 1], flow[:, :, 0]), dim=-1)
    return disp + pos_dev[None, None]


def _cvx_curve_trajectories(params, up_mask, bm, tile_size, H, W, scale, fused=False):
    """`_curve_trajectories` for control points on the 1/8 grid with their convex-upsampling mask (the RAFT-spline output head):
    on the GPU ops.CvxCurveTrajFn (csrc/cvx_curves.hip; tile sizes 2, 4, 8, 16), else the plain-torch mirror.  On the kernel route
    an fp16 / bf16 mask is passed as it is and gets its gradient in its own dtype (computed in fp32, rounded once); control points
    that are not fp32 go through a differentiable .float(); the basis matrix is fp32 and so are the trajectories."""
    B, c2, h, w = params.shape
    if up_mask.dim() != 4 or tuple(up_mask.shape) != (B, 576, h, w):
        raise ValueError(f'up_mask must be [B, 576, h, w] = {(B, 576, h, w)}, got {tuple(up_mask.shape)}')
    if (H, W) != (8 * h, 8 * w):
        raise ValueError(f'with up_mask, image_shape must be 8 x the grid of params: {(8 * h, 8 * w)}, got {(H, W)}')
    pos, pos_dev = _tile_positions(H, W, tile_size, params.device, params.dtype)
    if fused and _basis_trains(bm) and (H % tile_size or W % tile_size):
        fused = False                            # (the matrix' gradient reads the rows of mpc_pec_head_rows: whole tiles only)
    if _cvx_kernels_serve(params, up_mask, bm, fused) and tile_size in _CVX_KERNEL_TILES:
        from .. import ops
        return ops.CvxCurveTrajFn.apply(params.float(), up_mask, bm.float(), float(scale), int(tile_size)), pos
    return _cvx_curve_trajectories_mirror(params, up_mask, bm, pos_dev, scale), pos


def flows_from_bezier(params, times, up_mask=None, scale=1.0):
    """The dense flows of Bezier curves at `times`, [n_t, B, 2, H, W] in (x, y) order: with `up_mask` [B, 576, h, w] what the
    reference's `curve.create_upsampled(mask).get_flow_from_reference(times)` returns (curves/base.py:35-38, 95-123; evaluated per
    timestamp by src/modules/raft_spline.py:122-154) times `scale`, H x W = 8h x 8w; without it the flows of `params` on their own
    grid.  One kernel on the GPU (ops.cvx_flows) when nothing requires grad; plain torch (differentiable) otherwise."""
    B, c2, h, w = params.shape
    assert c2 % 2 == 0, params.shape
    d = c2 // 2
    bm = _device_basis('bernstein', times, (int(d),), params.device, _basis_dtype(params))    # [n_t, d]
    if up_mask is not None:
        if up_mask.dim() != 4 or tuple(up_mask.shape) != (B, 576, h, w):
            raise ValueError(f'up_mask must be [B, 576, h, w] = {(B, 576, h, w)}, got {tuple(up_mask.shape)}')
        needs_grad = torch.is_grad_enabled() and (params.requires_grad or up_mask.requires_grad)
        if not needs_grad and _cvx_kernels_serve(params, up_mask, bm):
            from .. import ops
            return ops.cvx_flows(params, up_mask, bm, float(scale))          # (fp32 flows; a 16-bit mask is read in place)
        params = _cvx_upsample(params, up_mask)
    return torch.einsum('bcdhw,td->tbchw', params.reshape(B, 2, d, *params.shape[-2:]), bm.to(params.dtype)) * scale


def bernstein_basis(times, degree):
    """[n_t] -> [n_t, degree]: C(d,i) (1-t)^(d-i) t^i for i = 1..d (P0 == 0), float64 then fp32.  (The caller's own copy: the cached
    matrix is shared by every later step.)"""
    return _cached_basis('bernstein', times, int(degree)).clone()


def _bernstein_basis_eval(times, degree):
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    out = np.zeros((t.size, degree))
    for d_idx in range(degree):
        i = d_idx + 1
        out[:, d_idx] = math.comb(degree, i) * (1 - t) ** (degree - i) * t ** i
    return torch.from_numpy(out).float()


def _polynomial_basis_eval(times, degree):
    """t^j for j = 1..d as the reference's PolynomialCurves evaluates it (curves/polynomial.py:55-58): the float64 times rounded to
    fp32, then an fp32 power (torch on the host)."""
    t = torch.from_numpy(np.asarray(times, dtype=np.float64).reshape(-1)).float()
    return t[:, None] ** torch.arange(1, degree + 1)[None, :]


def _polynomial_shortcut_basis_eval(times, degree):
    t = torch.from_numpy(np.asarray(times, dtype=np.float64).reshape(-1))
    return _shortcut_rows(_polynomial_basis_eval(t.numpy(), degree), t)


def _shortcut_rows(bm, t):
    """The scalar-time shortcuts of `CurveBase.get_flow_from_reference` (curves/base.py:98-106) as rows of the basis matrix: a time
    of exactly 0.0 gives zeros, a time of exactly 1.0 the last control point -- one-hot on the last column.  `t` holds the times
    as the caller gave them (the reference compares the Python float, base.py:102-105, BEFORE anything is rounded to fp32: a
    float64 time of 1 - 1e-12 gets no shortcut although it rounds to 1.0f), on the device of `bm` or the host.  Constants (no
    gradient reaches the basis network through them); elementwise, nothing is read back."""
    d = bm.shape[1]
    last = (torch.arange(d, device=bm.device) == d - 1).to(bm.dtype)          # (an indexed assignment of a scalar would synchronise)
    bm = torch.where((t == 1).to(bm.device)[:, None], last[None, :], bm)
    return torch.where((t == 0).to(bm.device)[:, None], torch.zeros((), dtype=bm.dtype, device=bm.device), bm)


CURVE_TYPES = ('BEZIER', 'POLYNOMIAL', 'LEARNED', 'BSPLINE')


def curve_basis(curve_type, times, degree, basis_network=None, scalar_time_shortcuts=False, device=None):
    """The [n_t, degree] fp32 basis matrix of one of the reference's three RAFT-spline curve types (`model.curve_type`, reference
    src/models/raft_spline/curves/__init__.py:13-21) or of the cubic B-spline, on `device` (default: that of the basis network's parameters for 'LEARNED', of
    `times` if it is a tensor, else the CPU): flow(t) = sum_j basis[t, j] * P_j.

      'BEZIER'      the Bernstein matrix of `trajectories_from_bezier` (bezier.py:92-113: float64 on the host, then fp32; the same
                    cached tensor, the same bits)
      'POLYNOMIAL'  times.float()[:, None] ** arange(1, d + 1), fp32 as curves/polynomial.py:55-58 evaluates it; cached per
                    timestamps tensor as the Bernstein matrix is (a training step neither synchronises nor uploads)
      'LEARNED'     basis_network(times.float()[:, None]) (curves/learned.py:76-77): part of the autograd graph, never cached; a
                    device `times` tensor causes no host synchronisation.  The learned basis is NOT zero at t = 0.
      'BSPLINE'     the cubic B-spline matrix of `trajectories_from_bspline` (`bspline_basis(times, degree + 1)`: float64 on the
                    host, then fp32; the same cached tensor, the same bits; degree >= 3) -- UNPINNED EXTENSION, the curve that
                    FocusLoss.calc_per_event_curves(curve_type='BSPLINE') evaluates per event
    Any other `curve_type` raises ValueError.  The cached matrices are shared: do not modify them in place.

    `scalar_time_shortcuts`: `CurveBase.get_flow_from_reference` returns the last control point for a SCALAR time == 1 and zeros
    for a scalar time == 0 whatever the curve type (curves/base.py:98-106); a list of times gets no shortcut.  For Bezier curves
    the two agree, for the other two types they do not.  False (the default): the list behaviour -- what the refinement loop
    (raft.py:178) and the loss evaluate.  True: a row whose time is exactly 0.0 is all zeros and a row whose time is exactly 1.0 is
    one-hot on the last column (compared as given -- a list or array as float64, a tensor in its own dtype --, before the rounding
    to fp32, as the reference compares the Python float), constants without gradient -- what `validation_step` evaluates, one scalar at a time
    (src/modules/raft_spline.py:134-154), and therefore the default of `trajectory_val_metrics` alone."""
    d = int(degree)
    if d < 1:
        raise ValueError(f'degree must be >= 1, got {degree}')
    if curve_type == 'LEARNED':
        if basis_network is None:
            raise ValueError("curve_type 'LEARNED' needs basis_network")
        if device is None:
            device = next((p.device for p in basis_network.parameters()), None)
        # t_in: the times as given (a tensor in its own dtype, anything else as float64), for the shortcut comparison
        t_in = times.detach().reshape(-1) if torch.is_tensor(times) else torch.from_numpy(np.asarray(times, dtype=np.float64).reshape(-1))
        t = t_in.to(device=device, dtype=torch.float32)
        bm = basis_network(t[:, None]).float()
        if bm.dim() != 2 or tuple(bm.shape) != (t.shape[0], d):
            raise ValueError(f'basis_network must map [n_t, 1] to [n_t, degree] = {(t.shape[0], d)}, got {tuple(bm.shape)}')
        return _shortcut_rows(bm, t_in) if scalar_time_shortcuts else bm
    if curve_type not in CURVE_TYPES:
        raise ValueError(f'curve_type must be one of {CURVE_TYPES}, got {curve_type!r}')
    if device is None:
        device = times.device if torch.is_tensor(times) else torch.device('cpu')
    if curve_type == 'BEZIER':                  # (the Bernstein rows at t = 0 and t = 1 ARE the shortcut rows: 0 ** 0 == 1)
        return _device_basis('bernstein', times, (d,), device, torch.float32)
    if curve_type == 'BSPLINE':                 # (clamped ends: its rows at t = 0 and t = 1 are the shortcut rows too)
        if d < BSPLINE_MIN_DEGREE:
            raise ValueError(f"curve_type='BSPLINE' is cubic: it needs degree >= {BSPLINE_MIN_DEGREE} control points per axis beside P0, got {d}")
        return _device_basis('bspline', times, (d + 1, 3), device, torch.float32)
    return _device_basis('polynomial_shortcuts' if scalar_time_shortcuts else 'polynomial', times, (d,), device, torch.float32)


def _curve_matrix(params, times, curve_type, basis_network):
    """(degree, the basis matrix of `curve_basis` on the device and in the dtype of `params`) for the entry points below."""
    c2 = params.shape[1]
    assert params.dim() == 4 and c2 % 2 == 0, params.shape
    return c2 // 2, curve_basis(curve_type, times, c2 // 2, basis_network, device=params.device).to(_basis_dtype(params))


def trajectories_from_curves(params, times, tile_size, image_shape, curve_type='BEZIER', basis_network=None, scale=1.0, up_mask=None,
                             basis_grad='mirror'):
    """`trajectories_from_bezier` for any of the reference's curve types (`curve_basis`: 'BEZIER' | 'POLYNOMIAL' | 'LEARNED', the
    latter with its `basis_network` on the device of `params`) and for 'BSPLINE' (the bits of `trajectories_from_bspline`): the same contracts, the same routing -- fp32, fp16 or bf16 GPU tensors (16-bit ones as `trajectories_from_bezier` says: the mask
    read in place, fp32 trajectories) with
    d <= 16 (and, with `up_mask`, a basis matrix within 48 KB and a tile size of 2, 4, 8 or 16) run in the fused nodes
    (ops.CurveTrajFn / ops.CvxCurveTrajFn), everything else in their plain-torch mirrors -- and with 'BEZIER' the same launches
    and bits.  Times are evaluated as a LIST (no scalar-time shortcut, see `curve_basis`): a learned curve is not zero at t = 0.
    Differentiable w.r.t. `params`, `up_mask` and, for 'LEARNED', the parameters of `basis_network`.  The fused nodes have no
    gradient for the basis matrix: a matrix that requires grad (a basis network that trains) takes the plain-torch mirrors, where it
    is an ordinary autograd input; a polynomial curve, and a learned one whose network is frozen or evaluated under no_grad, run in
    the fused nodes.

    `basis_grad` ('mirror', the default: the routing above, unchanged | 'fused'; anything else raises ValueError): with 'fused' a
    matrix that requires grad takes the fused nodes as well -- the launches of the frozen route and the same bits for the
    trajectories and for the gradients of `params` and `up_mask`, then the matrix' own gradient [n_t, d] in fp32 as a small
    deterministic reduction (csrc/curve_basis.hip: two kernels, behind one kernel that evaluates the upsampled control points at
    the tile centres with `up_mask`; no float atomics, no host synchronisation), from which autograd reaches the parameters of
    `basis_network` as it does from the mirror.  Shapes the kernels do not serve still take the mirror, and so does an
    `image_shape` that is no multiple of `tile_size` with `up_mask`.  With a constant matrix the keyword changes nothing."""
    fused = _basis_grad_fused(basis_grad)
    B, c2, h, w = params.shape
    H, W = (int(v) for v in image_shape)
    assert c2 % 2 == 0 and (up_mask is not None or (h == H // tile_size and w == W // tile_size)), (params.shape, image_shape, tile_size)
    d, bm = _curve_matrix(params, times, curve_type, basis_network)
    if up_mask is not None:
        return _cvx_curve_trajectories(params, up_mask, bm, tile_size, H, W, scale, fused)
    return _curve_trajectories(params, bm, tile_size, H, W, scale, fused)


def flows_from_curves(params, times, curve_type='BEZIER', basis_network=None, up_mask=None, scale=1.0):
    """`flows_from_bezier` for any of the reference's curve types (see `trajectories_from_curves`): [n_t, B, 2, H, W] in (x, y)
    order, the times evaluated as a LIST (no scalar-time shortcut).  One kernel on the GPU (ops.cvx_flows) when nothing requires
    grad -- the basis matrix of a learned curve included --, plain torch (differentiable) otherwise."""
    B, c2, h, w = params.shape
    d, bm = _curve_matrix(params, times, curve_type, basis_network)
    if up_mask is not None:
        if up_mask.dim() != 4 or tuple(up_mask.shape) != (B, 576, h, w):
            raise ValueError(f'up_mask must be [B, 576, h, w] = {(B, 576, h, w)}, got {tuple(up_mask.shape)}')
        needs_grad = torch.is_grad_enabled() and (params.requires_grad or up_mask.requires_grad)
        if not needs_grad and _cvx_kernels_serve(params, up_mask, bm):
            from .. import ops
            return ops.cvx_flows(params, up_mask, bm, float(scale))          # (fp32 flows; a 16-bit mask is read in place)
        params = _cvx_upsample(params, up_mask)
    return torch.einsum('bcdhw,td->tbchw', params.reshape(B, 2, d, *params.shape[-2:]), bm.to(params.dtype)) * scale


def trajectories_from_bezier(params, times, tile_size, image_shape, scale=1.0, up_mask=None):
    """RAFT-spline adapter: sample Bezier flow curves at the tile centres as `trajectories`
    for `FocusLoss.calc`.

    params [B, 2*d, h, w] with h = H // tile_size, w = W // tile_size, viewed [B, 2, d, h, w] with dim 1 in
    (x, y) order (reference src/models/raft_spline/curves/base.py:88-89, polynomial.py:60-61); the flow at time
    t is `CurveBase.get_flow_from_reference(t)` = sum_i B_i(t) P_i (bezier.py:92-113), which is zero at the
    anchor t = 0.  Returns (trajectories [B, n_t, n, 2] in (y, x) pixel coordinates, pixel_positions [n, 2]) with
    the tile centres of `get_optical_flow_tile_mask` as start points -- the layout `calc` expects
    (focus.py:66-72); `pixel_positions` is a cached tensor shared by all calls: do not modify it in place.  `scale` multiplies the flow (8.0 if the curve lives on RAFT's 1/8 grid units).
    Differentiable w.r.t. `params` (plain torch: 2*d*n_t multiply-adds per tile).

    With `up_mask` [B, 576, h, w] (the RAFT-spline output head: reference curves/base.py:35-38, raft_spline/utils.py:30-45) `params`
    are the control points on the 1/8 grid, `image_shape` must be (8h, 8w) (ValueError otherwise), and the curves are those of
    `BezierCurves(params).create_upsampled(up_mask)` sampled at the tile centres: the factor 8 of cvx_upsample is applied inside,
    `scale` multiplies on top.  Differentiable w.r.t. `params` and `up_mask`.

    fp16 / bf16 on the GPU (a network under autocast, a .half() / .bfloat16() model) within the kernels' limits takes the fused nodes:
    the mask is read in its own dtype (no .float() copy; the conversion at the load is exact) and its gradient comes back in that
    dtype, computed in fp32 and rounded once; control points that are not fp32 go through a differentiable .float(); basis matrix
    and tile positions are fp32.  The trajectories are then fp32 -- bit for bit those of the upcast inputs -- and NOT the 16-bit
    tensor the plain-torch mirror used to return for such inputs: displacement + pixel position in bf16 (8 significant bits) lies on
    a 2-4 px lattice between 256 and 640 px.  `FocusLoss.calc` converts its trajectories to fp32 anyway.  CPU tensors, and shapes
    beyond the kernels' limits, still take the mirrors in their own dtype."""
    B, c2, h, w = params.shape
    H, W = (int(v) for v in image_shape)
    assert c2 % 2 == 0 and (up_mask is not None or (h == H // tile_size and w == W // tile_size)), (params.shape, image_shape, tile_size)
    d = c2 // 2
    bm = _device_basis('bernstein', times, (int(d),), params.device, _basis_dtype(params))    # [n_t, d]
    if up_mask is not None:
        return _cvx_curve_trajectories(params, up_mask, bm, tile_size, H, W, scale)
    return _curve_trajectories(params, bm, tile_size, H, W, scale)


def bspline_basis(times, num_ctrl, degree=3):
    """[n_t] -> [n_t, num_ctrl - 1]: the clamped (open uniform) B-spline basis functions N_1 .. N_{m-1} of `degree` on [0, 1]
    (control point 0 is fixed at zero, as P0 of the reference's Bezier curves: the flow from the reference time vanishes at
    t = 0).  Cox-de Boor in float64, then fp32.  UNPINNED EXTENSION: the reference has no B-spline curve
    (src/models/raft_spline/curves holds Bezier and polynomial curves only) -- BASELINE.json's configs[3]
    names a cubic B-spline, so the basis is provided, default OFF, and checked against scipy.interpolate.BSpline."""
    return _cached_basis('bspline', times, int(num_ctrl), int(degree)).clone()          # (the caller's own copy)


def _bspline_basis_eval(times, num_ctrl, degree=3):
    m, p = int(num_ctrl), int(degree)
    assert m >= p + 1, 'need at least degree + 1 control points'
    t = np.clip(np.asarray(times, dtype=np.float64).reshape(-1), 0.0, 1.0)
    inner = np.linspace(0.0, 1.0, m - p + 1)
    knots = np.concatenate((np.zeros(p), inner, np.ones(p)))            # m + p + 1 knots
    # degree 0
    N = np.zeros((t.size, m + p))
    for i in range(m + p):
        lo, hi = knots[i], knots[i + 1]
        if hi > lo:
            N[:, i] = ((t >= lo) & (t < hi)) | ((t == 1.0) & (hi == 1.0))
    for q in range(1, p + 1):
        Nn = np.zeros((t.size, m + p - q))
        for i in range(m + p - q):
            a = knots[i + q] - knots[i]
            b = knots[i + q + 1] - knots[i + 1]
            if a > 0:
                Nn[:, i] += (t - knots[i]) / a * N[:, i]
            if b > 0:
                Nn[:, i] += (knots[i + q + 1] - t) / b * N[:, i + 1]
        N = Nn
    return torch.from_numpy(N[:, 1:m]).float()


# the host evaluators of `_cached_basis`, by kind
_BASIS_EVAL = {'bernstein': _bernstein_basis_eval, 'bspline': _bspline_basis_eval, 'polynomial': _polynomial_basis_eval,
               'polynomial_shortcuts': _polynomial_shortcut_basis_eval}


def trajectories_from_bspline(params, times, tile_size, image_shape, scale=1.0, degree=3, up_mask=None):
    """As trajectories_from_bezier (`up_mask` included), for a clamped uniform B-spline flow curve (cubic by default) with control
    points P_1 .. P_{m-1} = params [B, 2*(m-1), h, w] ((x, y) channel order) and P_0 = 0.  UNPINNED EXTENSION (see bspline_basis)."""
    B, c2, h, w = params.shape
    H, W = (int(v) for v in image_shape)
    assert c2 % 2 == 0 and (up_mask is not None or (h == H // tile_size and w == W // tile_size)), (params.shape, image_shape, tile_size)
    d = c2 // 2
    bm = _device_basis('bspline', times, (int(d + 1), int(degree)), params.device, _basis_dtype(params))      # [n_t, d]
    if up_mask is not None:
        return _cvx_curve_trajectories(params, up_mask, bm, tile_size, H, W, scale)
    return _curve_trajectories(params, bm, tile_size, H, W, scale)
