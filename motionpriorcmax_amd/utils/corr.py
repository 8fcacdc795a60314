"""The RAFT-spline correlation pyramid and its lookup (reference src/models/raft_spline/corr.py:125-348, raft_spline/utils.py:4-28;
the loop that calls it: raft.py:165-189).

`corr_pyramid` is the reference's batched matmul, division and average pools in plain torch: the mirror, the CPU path and the comparator.
`corr_pyramid_fused` builds the same pyramid on the GPU as one autograd node (ops.CorrPyramidFn, csrc/corr_pyramid.hip): every level
is its own fp32-MFMA GEMM against the pooled feature map, written once; fp16 / bf16 feature maps (the encoders under autocast) are read
in place, level 0 on the 16-bit matrix cores, and yield fp32 levels as raft.py:126 intends; inputs the kernels do not take -- CPU
tensors, other dtypes, non-contiguous tensors, D that is no multiple of 4 or above 512, more than 16 targets or 6 levels -- go to
`corr_pyramid`.  Both take one reference (tensors) or several (lists: the events-plus-frames pyramid of the reference's default model, ops.CorrPyramidMultiFn).
`CorrLookup` is the network's one gather, 12 times per forward: on the GPU one kernel each way (ops.CorrLookupFn, csrc/corr_lookup.hip); everything the kernels do not take --
CPU tensors, other dtypes, non-contiguous tensors, radius > 4, more than 16 targets or control points, more than 6 levels -- runs the
plain-torch mirror below, which is written as the reference's own operator chain (coordinate tensor, normalisation to [-1, 1],
grid_sample, cat / permute / reshape) and therefore also the comparator the probe times the kernels against."""
import torch
import torch.nn.functional as F

from .basis import _basis_grad_fused, _basis_served, _device_basis, curve_basis

_KERNEL_MAX_RADIUS, _KERNEL_MAX_TARGETS, _KERNEL_MAX_D, _KERNEL_MAX_LEVELS = 4, 16, 16, 6
_PYRAMID_DTYPES = (torch.float32, torch.float16, torch.bfloat16)         # what the pyramid kernels read in place (include/mpcmax.h: MPC_DT_*)


def _one_dtype(tensors):
    """The served feature maps of one call in ONE dtype: as they are where they share it (16-bit maps then go to the kernels in
    place), else the 16-bit ones through a differentiable .float() -- a map upcast by hand beside one that is not -- for the fp32
    node; each gradient still arrives in its input's dtype (the .float() node rounds it)."""
    if len({t.dtype for t in tensors}) == 1:
        return list(tensors)
    return [t if t.dtype == torch.float32 else t.float() for t in tensors]


def _levels_list(num_levels_per_target):
    if isinstance(num_levels_per_target, int):
        return [int(num_levels_per_target)]
    nl = [int(v) for v in num_levels_per_target]
    if not nl or min(nl) < 1:
        raise ValueError(f'num_levels_per_target must hold positive level counts, got {nl}')
    return nl


def level_target_indices(num_levels_per_target):
    """Host lists: level l holds the targets with num_levels >= l + 1, ascending (corr.py:296-302)."""
    nl = _levels_list(num_levels_per_target)
    return [[t for t, v in enumerate(nl) if v >= l + 1] for l in range(max(nl))]


def _pool_levels(corr, nl, B, h, w):
    """CorrData.get_downsampled per level (corr.py:106-123, 296-302) over the volume corr [n, B, h*w, h*w]."""
    tix = level_target_indices(nl)
    levels = [corr.reshape(len(nl), B * h * w, 1, h, w)]
    for l in range(1, len(tix)):
        prev = levels[-1]
        pick = [tix[l - 1].index(t) for t in tix[l]]
        sel = prev if len(pick) == prev.shape[0] else prev[pick]
        down = F.avg_pool2d(sel.reshape(-1, 1, *prev.shape[-2:]), 2, stride=2)
        levels.append(down.view(len(pick), B * h * w, 1, *down.shape[-2:]))
    return levels, tix


def _references(fmap1, fmap2, num_levels_per_target):
    """The list form checked: R tensors fmap1[r] [B, D, h, w], R tensors fmap2[r] [n_r, B, D, h, w] (4 dimensions: one target), R
    entries of level counts (an int or n_r ints) -> (fmap1, fmap2 as 5 dimensions, level counts as R lists).  All references
    share B, D, h, w (corr.py:171, 183)."""
    if not isinstance(fmap2, (list, tuple)) or not isinstance(num_levels_per_target, (list, tuple)) or \
            not len(fmap1) == len(fmap2) == len(num_levels_per_target) or not len(fmap1):
        raise ValueError('the list form takes as many fmap2 tensors and level-count entries as fmap1 tensors, one or more')
    f2s = [f[None] if f.dim() == 4 else f for f in fmap2]
    nls = [_levels_list(v) for v in num_levels_per_target]
    shape = tuple(fmap1[0].shape)
    for r, (f1, f2, nl) in enumerate(zip(fmap1, f2s, nls)):
        if f1.dim() != 4 or f2.dim() != 5 or tuple(f1.shape) != shape or tuple(f2.shape[1:]) != shape or len(nl) != f2.shape[0]:
            raise ValueError(f'reference {r}: fmap1 {tuple(f1.shape)}, fmap2 {tuple(f2.shape)} and {len(nl)} level counts do not belong '
                             f'together, or to the [B, D, h, w] = {shape} of reference 0')
    return list(fmap1), f2s, nls


def corr_pyramid(fmap1, fmap2, num_levels_per_target):
    """fmap1 [B, D, h, w], fmap2 [n, B, D, h, w] (or [B, D, h, w] for one target) -> (levels, target_indices): levels[l]
    [n_l, B*h*w, 1, h_l, w_l] = fmap1^T @ fmap2 / sqrt(D), 2 x 2 average-pooled l times (the pool drops an odd last row / column), for
    the targets of `level_target_indices` -- the reference's CorrComputation.get_correlation_volume and CorrData.get_downsampled
    (corr.py:262-270, 106-123) operator for operator.  target_indices are host lists.
    The list form -- fmap1 a list of R tensors, fmap2 a list of R tensors, num_levels_per_target a list of R entries (an int or a
    list of ints each) -- is the events-plus-frames pyramid (CorrComputation.__add__ and _corr_dot_prod_M_to_N, corr.py:221-225,
    246-260; events then frames in raft.py:131-144): the flat target list is the concatenation in the order given, and the volume
    the reference's expand / cat, one batched matmul and the division.  A list of one reference is the tensor form."""
    if isinstance(fmap1, (list, tuple)):
        f1s, f2s, nls = _references(fmap1, fmap2, num_levels_per_target)
        if len(f1s) == 1:
            return corr_pyramid(f1s[0], f2s[0], nls[0])
        B, D, h, w = f1s[0].shape
        nl = [v for ref in nls for v in ref]
        a = torch.cat([x.expand(len(ref), -1, -1, -1, -1) for x, ref in zip(f1s, nls)], dim=0)
        b = torch.cat(f2s, dim=0)
        corr = a.view(len(nl), B, D, h * w).transpose(-1, -2) @ b.view(len(nl), B, D, h * w)
        corr = corr / torch.sqrt(torch.tensor(D, device=corr.device).float())
        return _pool_levels(corr, nl, B, h, w)
    nl = _levels_list(num_levels_per_target)
    if fmap2.dim() == 4:
        fmap2 = fmap2[None]
    n, B, D, h, w = fmap2.shape
    if tuple(fmap1.shape) != (B, D, h, w) or len(nl) != n:
        raise ValueError(f'fmap1 {tuple(fmap1.shape)}, fmap2 {tuple(fmap2.shape)} and {len(nl)} level counts do not belong together')
    corr = fmap1.reshape(B, D, h * w).transpose(-1, -2) @ fmap2.reshape(n, B, D, h * w)
    corr = corr / torch.sqrt(torch.tensor(D, device=corr.device).float())
    return _pool_levels(corr, nl, B, h, w)


def _corr_pyramid_fused_refs(fmap1, fmap2, num_levels_per_target):
    f1s, f2s, nls = _references(fmap1, fmap2, num_levels_per_target)
    if len(f1s) == 1:
        return corr_pyramid_fused(f1s[0], f2s[0], nls[0])
    B, D, h, w = f1s[0].shape
    dev = f1s[0].device
    if not all(t.is_cuda and t.dtype in _PYRAMID_DTYPES and t.is_contiguous() and t.device == dev for t in f1s + f2s):
        return corr_pyramid(f1s, f2s, nls)
    import ctypes
    from .. import ops, _lib as C
    nl = [v for ref in nls for v in ref]
    if len(f1s) > C.CORR_MAX_REFS or len(nl) > C.CORR_MAX_TARGETS or max(nl) > C.CORR_MAX_LEVELS:
        return corr_pyramid(f1s, f2s, nls)
    desc, tix = ops.corr_pyramid_desc(B, h, w, nl)
    refs = ops.corr_pyramid_refs([len(ref) for ref in nls])
    if C.lib().mpc_corr_pyramid_multi_supported(ctypes.byref(desc), D, ctypes.byref(refs)) != 0:
        return corr_pyramid(f1s, f2s, nls)
    return list(ops.CorrPyramidMultiFn.apply(nls, *_one_dtype(f1s + f2s))), tix


def corr_pyramid_fused(fmap1, fmap2, num_levels_per_target):
    """`corr_pyramid` with the same arguments, checks, level shapes and target_indices, built on the GPU by ops.CorrPyramidFn where the
    kernels serve the inputs (fp32, fp16 or bf16, contiguous, CUDA, D a multiple of 4 up to 512, at most 16 targets and 6 levels):
    one autograd node with gradients to fmap1 and fmap2, no host synchronisation, bitwise reproducible.  Everything else returns
    `corr_pyramid(...)`.  Served 16-bit maps yield fp32 levels (what raft.py:126 intends with its `.float()`; `corr_pyramid` itself
    keeps the dtype of its input): where all maps of a call share one 16-bit dtype they are read in place -- level 0 on the 16-bit
    matrix cores, the same sum as on the upcast maps in another order; the levels above and both gradients the fp32 node's on the
    upcast maps bit for bit, the gradients rounded once to the maps' dtype --; where the dtypes are mixed the 16-bit ones go
    through a differentiable `.float()` and the fp32 node runs.  The list form (several references: events plus frames) goes to
    ops.CorrPyramidMultiFn under the same conditions on every tensor and on the merged target list, and at most 4 references (MPC_CORR_MAX_REFS): one node with the same
    launches, gradients to all 2R feature maps, equal bit for bit to the R single-reference nodes."""
    if isinstance(fmap1, (list, tuple)):
        return _corr_pyramid_fused_refs(fmap1, fmap2, num_levels_per_target)
    nl = _levels_list(num_levels_per_target)
    f2 = fmap2[None] if fmap2.dim() == 4 else fmap2
    if f2.dim() != 5:
        return corr_pyramid(fmap1, fmap2, nl)
    n, B, D, h, w = f2.shape
    if tuple(fmap1.shape) != (B, D, h, w) or len(nl) != n:
        raise ValueError(f'fmap1 {tuple(fmap1.shape)}, fmap2 {tuple(f2.shape)} and {len(nl)} level counts do not belong together')
    if not all(t.is_cuda and t.dtype in _PYRAMID_DTYPES and t.is_contiguous() and t.device == fmap1.device for t in (fmap1, f2)):
        return corr_pyramid(fmap1, fmap2, nl)
    import ctypes
    from .. import ops, _lib as C
    if n > C.CORR_MAX_TARGETS or max(nl) > C.CORR_MAX_LEVELS:
        return corr_pyramid(fmap1, fmap2, nl)
    desc, tix = ops.corr_pyramid_desc(B, h, w, nl)
    if C.lib().mpc_corr_pyramid_supported(ctypes.byref(desc), D) != 0:
        return corr_pyramid(fmap1, fmap2, nl)
    return list(ops.CorrPyramidFn.apply(*_one_dtype([fmap1, f2]), nl)), tix


def coords_grid(batch, ht, wd, device, dtype=torch.float32):
    """[batch, 2, ht, wd], channel 0 = x, channel 1 = y (raft_spline/utils.py:22-28)."""
    ys, xs = torch.meshgrid(torch.arange(ht, device=device), torch.arange(wd, device=device), indexing='ij')
    return torch.stack((xs, ys), dim=0).to(dtype)[None].repeat(batch, 1, 1, 1)


def _lookup_mirror(levels, target_indices, radius, coords):
    """corr.py:304-348 with bilinear_sampler (utils.py:4-20) written out: coords [T, B, 2, h, w] -> [B, E * K * K, h, w]."""
    coords = coords.permute(0, 1, 3, 4, 2)
    T, B, h1, w1, _ = coords.shape
    r = radius
    K = 2 * r + 1
    d = torch.linspace(-r, r, K, device=coords.device, dtype=coords.dtype)
    dy, dx = torch.meshgrid(d, d, indexing='ij')
    delta = torch.stack((dx, dy), dim=-1).view(1, K, K, 2)                     # [..., 0] = x offset (j - r), [..., 1] = y offset (i - r)
    out = []
    for l, (corr, tix) in enumerate(zip(levels, target_indices)):
        sel = coords if len(tix) == T else coords[tix]
        centroid = sel.reshape(len(tix) * B * h1 * w1, 1, 1, 2) / 2 ** l
        xg, yg = (centroid + delta).split([1, 1], dim=-1)
        H, W = corr.shape[-2:]
        grid = torch.cat((2 * xg / (W - 1) - 1, 2 * yg / (H - 1) - 1), dim=-1)
        feat = F.grid_sample(corr.reshape(-1, 1, H, W), grid, align_corners=True)
        out.append(feat.view(len(tix), B, h1, w1, K * K))
    out = torch.cat(out, dim=0).permute(1, 0, 4, 2, 3).reshape(B, -1, h1, w1)
    return out if out.dtype == torch.float64 else out.float()                  # (float64 stays: the tests measure the fp32 error against it)


class CorrLookup:
    """The lookup of CorrBlockParallelMultiTarget (corr.py:272-348) over a pyramid built elsewhere.

    levels[l] [n_l, B*h*w, 1, h_l, w_l] as `corr_pyramid` returns them; num_levels_per_target the host list that built them (level l
    holds the targets with more than l levels, ascending).  `lookup(coords)` / `__call__`: coords [T, B, 2, h, w] or a list of T
    tensors [B, 2, h, w] in (x, y) order -> [B, E * (2r+1)^2, h, w] fp32 in the reference's channel order: entries level-major, then
    by target within a level; inside an entry channel i * (2r+1) + j samples at (coords / 2^l) + (x: j - r, y: i - r), bilinear,
    align_corners=True, zero padding per tap.  `lookup_bezier(params, times)`: the reference's three lines
    `flows = bezier.get_flow_from_reference(times); coords1 = coords0 + flows; corr_block(coords1)` as one node.  Both are
    differentiable w.r.t. coords / params and every level that requires grad; only requested gradients are computed.
    A level below 2 x 2 raises ValueError (the reference divides by size - 1 there and returns NaN).

    `shared_grad=True` (opt-in; it applies where a level requires grad and the kernels serve the levels, and changes nothing
    elsewhere): the lookups of this object add their level cotangents into ONE set of gradient buffers, which the levels receive once
    per backward pass (ops.CorrGradGateFn / CorrLookupSharedFn), instead of one volume-sized gradient per lookup that autograd then
    sums.  Same values; the lookups' backwards must run on one stream (they do under loss.backward() / autograd.grad)."""

    def __init__(self, levels, num_levels_per_target, radius=4, shared_grad=False):
        self.levels = list(levels)
        self.num_levels_per_target = _levels_list(num_levels_per_target)
        self.target_indices = level_target_indices(self.num_levels_per_target)
        self.radius = int(radius)
        if self.radius < 1:
            raise ValueError(f'radius must be at least 1, got {radius}')
        if len(self.levels) != len(self.target_indices):
            raise ValueError(f'{len(self.levels)} levels given, the level counts {self.num_levels_per_target} need {len(self.target_indices)}')
        n0, bhw, one, h, w = self.levels[0].shape
        if one != 1 or bhw % (h * w):
            raise ValueError(f'level 0 must be [n, B*h*w, 1, h, w], got {tuple(self.levels[0].shape)}')
        self.B, self.h, self.w = bhw // (h * w), h, w
        for l, (lv, tix) in enumerate(zip(self.levels, self.target_indices)):
            if lv.dim() != 5 or tuple(lv.shape[:3]) != (len(tix), bhw, 1) or tuple(lv.shape[3:]) != (h >> l, w >> l):
                raise ValueError(f'level {l} must be {(len(tix), bhw, 1, h >> l, w >> l)}, got {tuple(lv.shape)}')
            if lv.shape[3] < 2 or lv.shape[4] < 2:
                raise ValueError(f'level {l} is {lv.shape[3]} x {lv.shape[4]}: a level below 2 x 2 cannot be sampled '
                                 '(align_corners=True divides by size - 1)')
        self.num_entries = sum(len(t) for t in self.target_indices)
        self._descs = {}
        self._bases = {}
        self.shared_grad = bool(shared_grad)
        self._gate = self._token = None
        if self.shared_grad and torch.is_grad_enabled() and any(lv.requires_grad for lv in self.levels) and self._levels_served():
            from .. import ops
            self._gate = ops.CorrGradGate()
            self._token = ops.CorrGradGateFn.apply(self._gate, *self.levels)

    @classmethod
    def from_block(cls, block, num_levels_per_target=None, shared_grad=False):
        """From the reference's CorrBlockParallelMultiTarget (duck-typed: block._corr_pyramid[i].corr, block._radius).  With
        `num_levels_per_target` (what the block's CorrComputation objects were built with, events then frames) nothing is read back
        from the device; without it the target indices are read from the block's device tensors
        (block._corr_pyramid[i].target_indices), which costs one device synchronisation."""
        pyramid = list(block._corr_pyramid)
        levels = [cd.corr for cd in pyramid]
        if num_levels_per_target is None:
            tix = torch.cat([torch.cat((cd.target_indices.reshape(-1), cd.target_indices.new_full((1,), -1))) for cd in pyramid]).tolist()
            n = levels[0].shape[0]
            num_levels_per_target = [0] * n
            for t in tix:
                if t >= 0:
                    num_levels_per_target[int(t)] += 1
        return cls(levels, num_levels_per_target, radius=int(block._radius), shared_grad=shared_grad)

    @classmethod
    def from_fmaps(cls, fmap1, fmap2, num_levels_per_target, radius=4, shared_grad=False):
        """The lookup over the pyramid of `corr_pyramid_fused(fmap1, fmap2, num_levels_per_target)`: what raft.py:129 / :161 build
        from the two feature maps, with the pyramid as one autograd node back to the feature maps.  In list form (fmap1, fmap2 and
        num_levels_per_target lists of R entries: raft.py:131-144 with boundary images, events then frames) the lookup is over the
        merged level counts.  fp16 / bf16 feature maps that the pyramid kernels serve give fp32 levels, so the lookups stay on
        their kernels."""
        levels, _ = corr_pyramid_fused(fmap1, fmap2, num_levels_per_target)
        if isinstance(fmap1, (list, tuple)):
            num_levels_per_target = [v for ref in num_levels_per_target for v in _levels_list(ref)]
        return cls(levels, num_levels_per_target, radius=radius, shared_grad=shared_grad)

    # ---- routing

    def _levels_served(self):
        dev = self.levels[0].device
        return (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in self.levels)
                and self.radius <= _KERNEL_MAX_RADIUS and len(self.num_levels_per_target) <= _KERNEL_MAX_TARGETS
                and len(self.levels) <= _KERNEL_MAX_LEVELS)

    def _apply(self, x, basis):
        from .. import ops
        if self._token is not None:                                             # shared_grad: the token stands in for the levels
            return ops.CorrLookupSharedFn.apply(x, basis, self, self._token)
        return ops.CorrLookupFn.apply(x, basis, self, *self.levels)

    def _kernels_serve(self, x, d):
        tensors = [x] + self.levels
        return (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device for t in tensors)
                and self.radius <= _KERNEL_MAX_RADIUS and len(self.num_levels_per_target) <= _KERNEL_MAX_TARGETS
                and d <= _KERNEL_MAX_D and len(self.levels) <= _KERNEL_MAX_LEVELS)

    def descriptor(self, d=0, flags=None):
        """The C descriptor (include/mpcmax.h: mpc_corr_desc) of this pyramid: built once per d, the kernels receive it by value."""
        from .. import _lib as C
        if flags is None:
            flags = getattr(self, 'flags', 0)
        key = (int(d), int(flags))
        desc = self._descs.get(key)
        if desc is None:
            desc = C.CorrDesc(B=self.B, h=self.h, w=self.w, T=len(self.num_levels_per_target), d=int(d), radius=self.radius,
                              num_levels=len(self.levels), flags=int(flags))
            for l, (lv, tix) in enumerate(zip(self.levels, self.target_indices)):
                desc.level_h[l], desc.level_w[l], desc.level_n[l] = lv.shape[3], lv.shape[4], len(tix)
                for s, t in enumerate(tix):
                    desc.level_target[l][s] = t
                desc.level[l] = lv.data_ptr()
            self._descs[key] = desc
        return desc

    def _basis(self, times, d, device, dtype, kind='bernstein'):
        if torch.is_tensor(times):
            return _device_basis(kind, times, (int(d),), device, dtype)
        key = (tuple(float(t) for t in times), int(d), device, dtype, kind)     # (a list: uploaded once per lookup object, not per call)
        bm = self._bases.get(key)
        if bm is None:
            bm = self._bases[key] = _device_basis(kind, list(key[0]), (int(d),), device, dtype)
        return bm

    # ---- the two calls

    def lookup(self, coords):
        if isinstance(coords, (list, tuple)):
            coords = torch.stack(tuple(coords), dim=0)
        T = len(self.num_levels_per_target)
        if coords.dim() != 5 or tuple(coords.shape) != (T, self.B, 2, self.h, self.w):
            raise ValueError(f'coords must be [T, B, 2, h, w] = {(T, self.B, 2, self.h, self.w)}, got {tuple(coords.shape)}')
        if self._kernels_serve(coords, 0):
            return self._apply(coords, None)
        return _lookup_mirror(self.levels, self.target_indices, self.radius, coords)

    __call__ = lookup

    def lookup_bezier(self, params, times):
        T = len(self.num_levels_per_target)
        if params.dim() != 4 or params.shape[1] % 2 or params.shape[1] < 2 or (params.shape[0], params.shape[2], params.shape[3]) != (self.B, self.h, self.w):
            raise ValueError(f'params must be [B, 2d, h, w] with (B, h, w) = {(self.B, self.h, self.w)}, got {tuple(params.shape)}')
        if len(times) != T:
            raise ValueError(f'{len(times)} times for {T} targets')
        d = params.shape[1] // 2
        bm = self._basis(times, d, params.device, params.dtype)                  # [T, d]
        if self._kernels_serve(params, d):
            return self._apply(params, bm)
        flows = torch.einsum('bcdhw,td->tbchw', params.reshape(self.B, 2, d, self.h, self.w), bm)
        coords = coords_grid(self.B, self.h, self.w, params.device, params.dtype)[None] + flows
        return _lookup_mirror(self.levels, self.target_indices, self.radius, coords)

    def lookup_curves(self, params, times, curve_type='BEZIER', basis_network=None, basis_grad='mirror'):
        """`lookup_bezier` for any of the reference's curve types (utils.curve_basis: 'BEZIER' | 'POLYNOMIAL' | 'LEARNED', the latter
        with its `basis_network` on the device of `params`; also 'BSPLINE', the cubic B-spline): the lookup at coords0 + curve.get_flow_from_reference(times) of
        raft.py:165-180, the times evaluated as a LIST (no scalar-time shortcut).  The same routing as `lookup_bezier`, with
        'BEZIER' the same launches and bits, `shared_grad=True` included.  For 'LEARNED' the basis matrix is part of the autograd
        graph, and the fused node has no gradient for it: while the basis network trains (the matrix requires grad) the lookup
        runs in the plain-torch mirror, where the matrix is an ordinary autograd input -- also when `params` are detached
        (`detach_bezier`, raft.py:166-167), which is what trains the basis network through the update loop.  A frozen network, or
        one evaluated under no_grad, runs in the fused node.

        `basis_grad` ('mirror', the default: the routing above, unchanged | 'fused'; anything else raises ValueError): with 'fused' a
        matrix that requires grad takes the fused node as well, `shared_grad=True` included -- the forward and backward launches of
        the frozen route and the same bits for the output and for the gradients of `params` and the levels; the backward launch
        also writes the targets' coordinate gradient [T, B, 2, h, w] (alone, without the gradient of `params`, where they are
        detached), from which two small kernels sum the matrix' gradient [T, d] in a fixed order (csrc/curve_basis.hip: no float
        atomics, no host synchronisation).  Autograd carries it into the parameters of `basis_network`."""
        fused = _basis_grad_fused(basis_grad)
        T = len(self.num_levels_per_target)
        if params.dim() != 4 or params.shape[1] % 2 or params.shape[1] < 2 or (params.shape[0], params.shape[2], params.shape[3]) != (self.B, self.h, self.w):
            raise ValueError(f'params must be [B, 2d, h, w] with (B, h, w) = {(self.B, self.h, self.w)}, got {tuple(params.shape)}')
        if len(times) != T:
            raise ValueError(f'{len(times)} times for {T} targets')
        d = params.shape[1] // 2
        if curve_type in ('BEZIER', 'POLYNOMIAL'):
            bm = self._basis(times, d, params.device, params.dtype, 'bernstein' if curve_type == 'BEZIER' else 'polynomial')
        else:                                    # (the network's output, as it comes: the kernel reads a dense [T, d])
            bm = curve_basis(curve_type, times, d, basis_network, device=params.device).to(params.dtype).contiguous()
        if self._kernels_serve(params, d) and _basis_served(bm, fused):
            return self._apply(params, bm)
        flows = torch.einsum('bcdhw,td->tbchw', params.reshape(self.B, 2, d, self.h, self.w), bm)
        coords = coords_grid(self.B, self.h, self.w, params.device, params.dtype)[None] + flows
        return _lookup_mirror(self.levels, self.target_indices, self.radius, coords)
