"""Cases, exact references, a restatement of the kernels' index arithmetic and the comparator for the RAFT-spline output head
(csrc/cvx_curves.hip, csrc/cvx_device.h), shared by tests/test_cvx_cases_host.py (CPU) and tests/test_gpu_cvx_cases.py.

Selector inputs, for which all of the head's arithmetic is exact.  The logits are 0 or -1000 (exp(-1000) is exactly 0 in fp32 and in
float64) with m in {1, 2, 4, 8} zeros among the nine of a pixel, so every weight is 0 or exactly 1/m; the control points are integers
in [-3, 3], the basis matrix is randint(-8, 9) / 8, scale = 0.5 and the cotangents are integers in [-2, 2].  Every product and every
partial sum of any order is then a multiple of a small power of two (UNIT below, per output, derived there), and `expected` asserts
for every output that A / UNIT < 2^24 with A the same expression on absolute values, and that the float64 value is representable in
fp32.  So whatever the order of the sums, traj, flows, dflow, the weights, grad_mask and grad_params have to equal the float64
evaluation bit for bit (torch.equal: -0 equals +0, a zero weight times a finite number may carry either sign).

`evaluate` is the head's formula in float64 from given weights (the softmax of the logits unless others are handed in: the weighted
device test evaluates everything after the weights from the device's own), on values or on absolute values.  `restated` is a NumPy
float64 restatement of the four kernels thread by thread -- the thread-to-centre decode, cvx_is_centre, the zero fill's plane / chunk /
element walk with its `uni` shortcut and its two store forms, the gather ranges of k_cvx_bwd_params, the staged basis -- that writes
into arrays prefilled with NaN, returns a census of the paths a case takes and serves the named mutants of MUTANTS."""
import math
import types

import numpy as np
import torch

U = 2.0 ** -24
SCALE = 0.5
FILL_ELEMS = 1024                                       # CVX_FILL_ELEMS

# name -> B, d, h, w, tile, T
_SPECS = dict(
    onehot_border=(2, 3, 2, 3, 4, 3),
    tile1_row=(2, 10, 1, 7, 1, 8),
    tile2=(1, 2, 3, 4, 2, 2),
    tile8=(1, 4, 3, 5, 8, 2),
    tile3=(2, 5, 3, 5, 3, 3),
    tile5_d11=(1, 11, 2, 3, 5, 24),
    tile16_d16=(1, 16, 3, 4, 16, 33),
    tile32_one=(1, 4, 5, 5, 32, 2),
    tile32_none=(1, 4, 5, 2, 32, 2),
    plane1025_t4=(2, 1, 25, 41, 4, 1),
    plane1025_t16=(2, 1, 25, 41, 16, 1),
    plane2052_t4=(1, 1, 27, 76, 4, 1),
    workload_plane=(1, 2, 60, 80, 4, 2),
)
CASES = tuple(n for n in _SPECS if n != 'workload_plane')
LARGE = 'workload_plane'                                # the workload's own plane: five fill chunks, the last one partial
OUTPUTS = ('traj', 'flows', 'dflow', 'weights', 'grad_mask', 'grad_params')
MUTANTS = ('k_transposed', 'pad_clamped', 'sy_sx_swapped', 'xy_swapped', 'centre_floor', 'gather_same_k', 'gather_hi_unclipped',
           'fill_first_chunk_only', 'fill_uni_always', 'basis_first_256', 'sample_stride_n_rounded')

# The smallest power of two every partial result of an output is a multiple of, with w in {0, 1, 1/2, 1/4, 1/8} (2^-3), 8 * params a
# multiple of 2^3, the basis a multiple of 2^-3, integer cotangents and scale = 2^-1:
#   up = sum w * (8 p): 2^0;  flows = (sum basis * up) * scale: 2^-3, then 2^-4;  traj = pos + flows: 2^-4
#   dflow = (sum basis * g) * scale: 2^-3, then 2^-4
#   g9 = sum (8 p) * dflow: 2^-1;  dot = sum w * g9: 2^-4;  grad_mask = w * (g9 - dot): 2^-7
#   grad_params = 8 * sum w * dflow: 2^-7 inside the sum
UNIT = dict(traj=2.0 ** -4, flows=2.0 ** -4, dflow=2.0 ** -4, weights=2.0 ** -3, grad_mask=2.0 ** -7, grad_params=2.0 ** -7)


def gamma(n):
    return n * U / (1.0 - n * U)


def tiles(v8, tile):
    """cvx_tiles: the tile centres tile / 2 + i * tile below v8."""
    s = tile >> 1
    return (v8 - s + tile - 1) // tile if v8 > s else 0


def roundings(name_or_case):
    """N_X, the fp32 roundings on the longest path from a weight or an input to an element of X, counted from the kernels (an add
    to the initial 0.f and the products 8.f * p are exact and not counted):
      up (cvx_up)      1 product + 8 adds                                      = 9
      flows            up, 1 product, d - 1 adds, the product with scale       = d + 10
      traj             flows, the add of the centre                            = d + 11
      dflow            1 product, T - 1 adds, the product with scale           = T + 1
      grad_mask        dflow, g9: 1 product + 2d - 1 adds, dot: 1 product + 8 adds, the difference, the product with w_k
                                                                               = N_dflow + 2d + 11
      grad_params      dflow, 1 product, 9 * ceil(8 / tile)^2 - 1 adds (nine cells of at most ceil(8 / tile)^2 centres each; the
                       final 8.f * acc is exact)                               = N_dflow + 9 * ceil(8 / tile)^2
    Every term of an output passes through at most N factors (1 + delta), |delta| <= 2^-24, so |X_fp32 - X| <= gamma(N) * A_X."""
    cs = case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    nd = cs.T + 1
    return dict(flows=cs.d + 10, traj=cs.d + 11, dflow=nd, grad_mask=nd + 2 * cs.d + 11, grad_params=nd + 9 * (-(-8 // cs.tile)) ** 2)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
_CASE = {}


def make_case(name, B, d, h, w, tile, T, params, mask, basis, g, scale):
    nty, ntx = tiles(8 * h, tile), tiles(8 * w, tile)
    s = tile >> 1
    ys, xs = s + tile * torch.arange(nty), s + tile * torch.arange(ntx)
    pos = torch.stack((ys[:, None].expand(nty, ntx), xs[None].expand(nty, ntx)), dim=-1).reshape(nty * ntx, 2)
    assert tuple(params.shape) == (B, 2 * d, h, w) and tuple(mask.shape) == (B, 576, h, w) and tuple(basis.shape) == (T, d)
    assert tuple(g.shape) == (B, T, nty * ntx, 2)
    return types.SimpleNamespace(name=name, B=B, d=d, h=h, w=w, tile=tile, T=T, nty=nty, ntx=ntx, n=nty * ntx, plane=h * w, pos=pos,
                                 params=params, mask=mask, basis=basis, g=g, scale=scale)


def case(name):
    """params [B, 2d, h, w], mask [B, 576, h, w], basis [T, d], g [B, T, n, 2]: fp32 on the CPU, seeded per case."""
    if name not in _CASE:
        B, d, h, w, tile, T = _SPECS[name]
        gen = torch.Generator().manual_seed(11 + 7919 * list(_SPECS).index(name))
        if name == 'onehot_border':                       # m = 1 and every k at every cell: k walks with the subpixel, the cell and b
            sub = torch.arange(64).reshape(1, 8, 8, 1, 1) + torch.arange(h * w).reshape(1, 1, 1, h, w) + 4 * torch.arange(B).reshape(B, 1, 1, 1, 1)
            zeros = (sub % 9)[:, None] == torch.arange(9).reshape(1, 9, 1, 1, 1, 1)
        else:
            m = torch.tensor([1, 2, 4, 8])[torch.randint(0, 4, (B, 1, 8, 8, h, w), generator=gen)]
            rank = torch.rand(B, 9, 8, 8, h, w, generator=gen).argsort(dim=1).argsort(dim=1)
            zeros = rank < m
        mask = torch.where(zeros, 0.0, -1000.0).float().reshape(B, 576, h, w)
        params = torch.randint(-3, 4, (B, 2 * d, h, w), generator=gen).float()
        basis = torch.randint(-8, 9, (T, d), generator=gen).float() / 8.0
        n = tiles(8 * h, tile) * tiles(8 * w, tile)
        g = torch.randint(-2, 3, (B, T, n, 2), generator=gen).float()
        _CASE[name] = make_case(name, B, d, h, w, tile, T, params, mask, basis, g, SCALE)
    return _CASE[name]


# ---- the formula in float64 -------------------------------------------------------------------------------------------------------
def softmax64(mask):
    """[B, 576, h, w] -> the float64 weights [B, 9, 8, 8, h, w] (k, sy, sx, cy, cx)."""
    B, _, h, w = mask.shape
    return torch.softmax(mask.double().reshape(B, 9, 8, 8, h, w), dim=1)


def dense_weights(per_pixel, h, w):
    """[B, 9, 64 h w] per pixel y * 8w + x (what a tile-1 backward leaves in its workspace) -> [B, 9, 8, 8, h, w]."""
    B = per_pixel.shape[0]
    return per_pixel.reshape(B, 9, h, 8, w, 8).permute(0, 1, 3, 5, 2, 4).contiguous()


def evaluate(cs, wts=None, absolute=False):
    """The head from the weights [B, 9, 8, 8, h, w] on, in float64: flows [T, B, 2, 8h, 8w] ((x, y)), traj [B, T, n, 2] ((y, x)),
    dflow [B, 2d, n], weights [B, 9, n] (at the centres), grad_mask [B, 576, h, w], grad_params [B, 2d, h, w].  absolute: the same
    expressions with every input and every term replaced by its absolute value (A_X)."""
    B, d, h, w, T, n = cs.B, cs.d, cs.h, cs.w, cs.T, cs.n
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    wts = softmax64(cs.mask) if wts is None else wts.double()
    p, bm, g = ab(cs.params.double()), ab(cs.basis.double()), ab(cs.g.double())
    p8 = torch.nn.functional.pad(8.0 * p, (1, 1, 1, 1))
    nb = torch.stack([p8[:, :, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], dim=2)            # [B, 2d, 9, h, w]
    up = (wts[:, None] * nb[:, :, :, None, None]).sum(dim=2)                                              # [B, 2d, 8, 8, h, w]
    up = up.permute(0, 1, 4, 2, 5, 3).reshape(B, 2, d, 8 * h, 8 * w)
    flows = torch.einsum('bcjhw,tj->tbchw', up, bm) * cs.scale
    py, px = cs.pos[:, 0], cs.pos[:, 1]
    at = flows[:, :, :, py, px]                                                                           # [T, B, 2, n]
    traj = torch.stack((at[:, :, 1], at[:, :, 0]), dim=-1).permute(1, 0, 2, 3) + cs.pos.double()[None, None]
    dflow = torch.cat((torch.einsum('btn,tj->bjn', g[..., 1], bm), torch.einsum('btn,tj->bjn', g[..., 0], bm)), dim=1) * cs.scale
    cy, sy, cx, sx = py // 8, py % 8, px // 8, px % 8
    wc = wts[:, :, sy, sx, cy, cx]                                                                        # [B, 9, n]
    g9 = (nb[:, :, :, cy, cx] * dflow[:, :, None]).sum(dim=1)                                             # [B, 9, n]
    dot = (wc * g9).sum(dim=1, keepdim=True)
    gm = torch.zeros(B, 9, 8, 8, h, w, dtype=torch.float64)
    gm[:, :, sy, sx, cy, cx] = wc * (g9 + dot if absolute else g9 - dot)
    gp = torch.zeros(B, 2 * d, (h + 2) * (w + 2), dtype=torch.float64)
    for k in range(9):
        gp.index_add_(2, (cy + k // 3) * (w + 2) + cx + k % 3, 8.0 * wc[:, None, k] * dflow)
    gp = gp.reshape(B, 2 * d, h + 2, w + 2)[:, :, 1:h + 1, 1:w + 1].contiguous()
    return types.SimpleNamespace(flows=flows, traj=traj, dflow=dflow, weights=wc, grad_mask=gm.reshape(B, 576, h, w), grad_params=gp)


def autograd64(cs):
    """traj, flows and the two gradients through the plain-torch mirror of utils/basis.py in float64."""
    from motionpriorcmax_amd.utils import basis as UB
    p, m = cs.params.double().requires_grad_(True), cs.mask.double().requires_grad_(True)
    bm = cs.basis.double()
    traj = UB._cvx_curve_trajectories_mirror(p, m, bm, cs.pos.double(), cs.scale)
    gp, gm = torch.autograd.grad(traj, [p, m], cs.g.double())
    up = UB._cvx_upsample(p.detach(), m.detach())
    flows = torch.einsum('bcdhw,td->tbchw', up.reshape(cs.B, 2, cs.d, 8 * cs.h, 8 * cs.w), bm) * cs.scale
    return types.SimpleNamespace(traj=traj.detach(), flows=flows, grad_params=gp, grad_mask=gm)


_EXPECTED = {}
RATIO = {}                                              # case -> {output: A / UNIT / 2^24} (printed by the host test)


def exact(cs):
    """The float64 evaluation of a selector case as fp32 tensors, after the exactness assertions: for every output A / UNIT < 2^24,
    every value a multiple of its UNIT and representable in fp32.  -> the tensors, {output: A / UNIT / 2^24}."""
    val, mag = evaluate(cs), evaluate(cs, absolute=True)
    ratio, out = {}, {}
    for k in OUTPUTS:
        v, a = getattr(val, k), getattr(mag, k)
        ratio[k] = float(a.max()) / UNIT[k] / 2.0 ** 24 if a.numel() else 0.0
        assert ratio[k] < 1.0, (cs.name, k, ratio[k])
        assert bool((v.abs() <= a).all()) and torch.equal(v / UNIT[k], (v / UNIT[k]).round()), (cs.name, k)
        assert torch.equal(v.float().double(), v), f'{cs.name} {k}: the float64 value is not representable in fp32'
        out[k] = v.float()
    return types.SimpleNamespace(**out), ratio


def expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name], RATIO[name] = exact(case(name))
    return _EXPECTED[name]


# ---- the cases of the other routes ------------------------------------------------------------------------------------------------
TIMES = [0.41, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0, 1.0]          # tools/gen_golden_cvx.py: t_ref, five bin mid-times, the two ends
HEAD_ROWS_CASES = ('onehot_border', 'tile2', 'tile8', 'plane1025_t4', 'plane2052_t4')     # tile 2, 4, 8 or 16 dividing 8h and 8w
WEIGHTED_SHAPES = dict(tile1_row=None, tile3=None, tile5_d11=None, tile16_d16=None, plane1025_t4=None, golden_a=(2, 10, 2, 3, 4))
WEIGHTED_VARIANTS = ('grid', 'times30', 'ties')


def _matrix(kind, d):
    from motionpriorcmax_amd import utils
    times = torch.tensor(TIMES, dtype=torch.float64)
    return (utils.bernstein_basis(times, d) if kind == 'bernstein' else utils.bspline_basis(times, d + 1)).float()


def with_matrix(name, kind='bernstein'):
    """A selector case under a real basis matrix at TIMES (T = 8, what the public functions build), with integer cotangents of its
    own: the raw entry points and the public route are compared with each other on it."""
    cs = case(name)
    gen = torch.Generator().manual_seed(5 + list(_SPECS).index(name))
    g = torch.randint(-2, 3, (cs.B, len(TIMES), cs.n, 2), generator=gen).float()
    return make_case(f'{name} ({kind})', cs.B, cs.d, cs.h, cs.w, cs.tile, len(TIMES), cs.params, cs.mask, _matrix(kind, cs.d), g, cs.scale)


def head_rows_case(name):
    """mpc_pec_head_rows / _bwd on a selector case: the head with the identity as its matrix (T = d), rows [B * n, 2d] = scale *
    (up_y, up_x) at the centres, an integer cotangent on the rows.  -> the case, its exact outputs, rows, grad_rows (fp32)."""
    cs = case(name)
    B, d, n = cs.B, cs.d, cs.n
    gen = torch.Generator().manual_seed(3 + list(_SPECS).index(name))
    g_rows = torch.randint(-2, 3, (B * n, 2 * d), generator=gen).float()
    g = torch.stack((g_rows[:, :d], g_rows[:, d:]), dim=-1).reshape(B, n, d, 2).permute(0, 2, 1, 3).contiguous()    # [B, T = d, n, (y, x)]
    hc = make_case(f'{name} (head rows)', B, d, cs.h, cs.w, cs.tile, d, cs.params, cs.mask, torch.eye(d), g, cs.scale)
    e, _ = exact(hc)
    disp = e.traj - hc.pos.float()[None, None]                                                 # [B, d, n, (y, x)]: exact, as asserted
    rows = torch.cat((disp[..., 0], disp[..., 1]), dim=1).permute(0, 2, 1).reshape(B * n, 2 * d)
    return hc, e, rows, g_rows


def weighted(shape, variant):
    """An inexact case on one of WEIGHTED_SHAPES: logits on a grid of 1/16 in [-8, 8] (`grid`; wk - mx is exact then and only expf,
    the nine-term sum and the division round), the same times 30 (`times30`), or all nine logits equal at half of the pixels and 3,
    5, 6, 7 or 9 zeros among -1000s at the others (`ties`); control points randn * 0.5, cotangents randn, scale 1.5; the Bernstein
    matrix at TIMES, for `times30` the cubic B-spline matrix where d >= 3."""
    B, d, h, w, tile = WEIGHTED_SHAPES[shape] or _SPECS[shape][:5]
    gen = torch.Generator().manual_seed(1000 + 31 * list(WEIGHTED_SHAPES).index(shape) + WEIGHTED_VARIANTS.index(variant))
    if variant == 'ties':
        m = torch.tensor([3, 5, 6, 7, 9])[torch.randint(0, 5, (B, 1, 8, 8, h, w), generator=gen)]
        rank = torch.rand(B, 9, 8, 8, h, w, generator=gen).argsort(dim=1).argsort(dim=1)
        level = torch.randint(-128, 129, (B, 1, 8, 8, h, w), generator=gen).float() / 16.0
        tie = torch.rand(B, 1, 8, 8, h, w, generator=gen) < 0.5
        mask = torch.where(tie, level.expand(B, 9, 8, 8, h, w), torch.where(rank < m, 0.0, -1000.0)).float()
    else:
        mask = torch.randint(-128, 129, (B, 9, 8, 8, h, w), generator=gen).float() / 16.0 * (30.0 if variant == 'times30' else 1.0)
    params = torch.randn(B, 2 * d, h, w, generator=gen) * 0.5
    n = tiles(8 * h, tile) * tiles(8 * w, tile)
    g = torch.randn(B, len(TIMES), n, 2, generator=gen)
    kind = 'bspline' if variant == 'times30' and d >= 3 else 'bernstein'
    return make_case(f'{shape} {variant}', B, d, h, w, tile, len(TIMES), params, mask.reshape(B, 576, h, w), _matrix(kind, d), g, 1.5)


MIN_NORMAL = 2.0 ** -126
UNDERFLOW = 2.0 ** -100                                  # see stage2_bounds


def weight_error(wts, mask):
    """The largest error of fp32 weights [B, 9, 8, 8, h, w] against the float64 softmax of the logits, per element and relative to
    the float64 weight -- to the smallest normal fp32 number where the weight is below it (expf(-1000) is 0, and so it should be)."""
    w64 = softmax64(mask)
    return float(((wts.double() - w64).abs() / w64.clamp(min=MIN_NORMAL)).max())


def stage2_bounds(cs, wts):
    """Everything after the weights, in float64 from the given fp32 weights: -> {output: (X64, gamma(N_X) * A_X)} with N_X of
    roundings().  Where A_X > 0 the bound gets UNDERFLOW = 2^-100 on top: a product with a subnormal weight (logits 480 apart) is
    rounded, or flushed, to within 2^-126 absolutely, not relatively, and fewer than 2^10 such results, each scaled by later factors
    below 2^10, meet in an element.  An element with A_X = 0 keeps the bound 0: it has to be exactly 0."""
    val, mag, N = evaluate(cs, wts), evaluate(cs, wts, absolute=True), roundings(cs)
    out = {}
    for k, nk in N.items():
        a = getattr(mag, k)
        out[k] = (getattr(val, k), gamma(nk) * a + torch.where(a > 0, UNDERFLOW, 0.0))
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def compare(label, output, got, want, bound=None):
    """bound None: `got` (fp32) equals `want` (fp32) as torch.equal has it, so -0 equals +0 and a NaN equals nothing; else
    |got - want| <= bound per element, with want and bound float64, and an element whose bound is 0 has to be exactly 0.  Raises an
    AssertionError that names the first bad element by its index with both values.  -> the largest error / bound."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (label, output, got.dtype, tuple(got.shape), tuple(want.shape))
    ratio = 0.0
    if bound is None:
        assert want.dtype == torch.float32
        bad = ~(got == want)
    else:
        assert want.dtype == torch.float64 and bound.dtype == torch.float64 and bool((bound >= 0).all())
        err = (got.double() - want).abs()
        bad = ~(err <= bound)
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    nbad = int(bad.sum())
    if nbad or not math.isfinite(ratio):
        ratio = float('inf')
    print(f'{label} {output}: {"bit for bit" if bound is None else f"largest error / bound {ratio:.4f}"}, {got.numel()} elements', flush=True)
    if nbad:
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        tail = '' if bound is None else f', |difference| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e}'
        raise AssertionError(f'{label} {output}: first bad element {idx}: got {float(got[idx])!r}, expected {float(want[idx])!r}{tail} '
                             f'({nbad} of {bad.numel()} bad)')
    return ratio


def compare_all(label, name, **outputs):
    """Whatever is given of OUTPUTS against expected(name), bit for bit."""
    e = expected(name)
    for k, v in outputs.items():
        compare(label, k, v, getattr(e, k))


# ---- the kernels, restated --------------------------------------------------------------------------------------------------------
def _is_centre(v, s, tile):
    return (v >= s) & ((v - s) % tile == 0)


def restated(name, mutant=None, base_offset=0):
    """k_cvx_traj_fwd, k_cvx_flow_fwd, k_cvx_bwd_centres (both roles) and k_cvx_bwd_params thread by thread in float64, vectorised
    over the threads of a launch.  base_offset: the float offset of grad_mask from a 16-byte boundary (decides the store form of the
    fill, nothing else).  -> traj, flows, dflow, weights, grad_mask, grad_params as fp32 tensors (NaN where no thread wrote) and
    `census`, the set of paths taken."""
    assert mutant is None or mutant in MUTANTS
    cs = case(name)
    B, d, T, h, w, tile, nty, ntx, n, plane = cs.B, cs.d, cs.T, cs.h, cs.w, cs.tile, cs.nty, cs.ntx, cs.n, cs.plane
    P = cs.params.double().numpy().reshape(B, 2 * d, plane)
    M = cs.mask.double().numpy().reshape(B, 576, plane)
    G = cs.g.double().numpy()
    scale = cs.scale
    s = (tile - 1) >> 1 if mutant == 'centre_floor' else tile >> 1           # the kernels' tile >> 1 (the host's counts are cvx_tiles')
    census = set()
    nan = float('nan')

    # the staged basis: thread i of 256 copies elements i, i + 256, ...
    sb = np.full(T * d, nan)
    passes = 0
    for i0 in range(0, T * d, 256):
        i = i0 + np.arange(256)
        i = i[i < T * d]
        sb[i] = cs.basis.double().numpy().reshape(-1)[i]
        passes += 1
        if mutant == 'basis_first_256':
            break
    sb = sb.reshape(T, d)
    census.add(('basis_passes', passes))
    census.add(('template', 4 if d <= 4 else 10 if d <= 10 else 16, d))

    def softmax9(b, y, x):
        cy, sy, cx, sx = y >> 3, y & 7, x >> 3, x & 7
        ch = sx * 8 + sy if mutant == 'sy_sx_swapped' else sy * 8 + sx
        lg = M[b[None], np.arange(9)[:, None] * 64 + ch[None], (cy * w + cx)[None]]          # [9, N]
        e = np.exp(lg - lg.max(axis=0))
        return e / e.sum(axis=0), ch

    def neighbour(k, cy, cx):
        dy, dx = (k % 3 - 1, k // 3 - 1) if mutant == 'k_transposed' else (k // 3 - 1, k % 3 - 1)
        ny, nx = cy + dy, cx + dx
        inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        cell = np.clip(ny, 0, h - 1) * w + np.clip(nx, 0, w - 1)
        return ny, nx, inside, (np.ones_like(inside) if mutant == 'pad_clamped' else inside), cell

    def up(b, y, x):                                      # cvx_up -> ux, uy [d, N]
        wk, _ = softmax9(b, y, x)
        cy, cx = y >> 3, x >> 3
        u = np.zeros((2 * d, y.size))
        for k in range(9):
            ny, nx, inside, use, cell = neighbour(k, cy, cx)
            sel = wk[k] > 0
            for side, hit in (('top', ny < 0), ('bottom', ny >= h), ('left', nx < 0), ('right', nx >= w)):
                if bool((sel & hit).any()):
                    census.add(('pad', side, k))
            u = u + np.where(use, wk[k] * (8.0 * P[b[None], np.arange(2 * d)[:, None], cell[None]]), 0.0)
        return (u[d:], u[:d]) if mutant == 'xy_swapped' else (u[:d], u[d:])

    def centre_threads():                                 # gi -> (b, i, y, x) of the threads that pass `gi >= B * n`
        gi = np.arange(-(-B * n // 256) * 256)
        gi = gi[gi < B * n]
        nn = -(-n // 256) * 256 if mutant == 'sample_stride_n_rounded' else max(n, 1)
        b = gi // nn
        i = gi - b * nn
        wg = gi // 256
        if bool(((wg[1:] == wg[:-1]) & (b[1:] != b[:-1])).any()):
            census.add('workgroup_spans_two_samples')
        ok = (i < n) & (b < B)                            # (only the mutant fails this)
        b, i = b[ok], i[ok]
        iy = i // ntx
        ix = i - iy * ntx
        return b, i, s + iy * tile, s + ix * tile

    # ---- k_cvx_traj_fwd
    traj = np.full((B, T, n, 2), nan)
    if B * n:
        b, i, y, x = centre_threads()
        ux, uy = up(b, y, x)
        for t in range(T):
            traj[b, t, i, 0] = y + (sb[t][:, None] * uy).sum(axis=0) * scale
            traj[b, t, i, 1] = x + (sb[t][:, None] * ux).sum(axis=0) * scale

    # ---- k_cvx_flow_fwd: one thread per pixel
    H, W, HW = 8 * h, 8 * w, 64 * plane
    flows = np.full((T, B, 2, HW), nan)
    gi = np.arange(-(-B * HW // 256) * 256)
    gi = gi[gi < B * HW]
    b = gi // HW
    pix = gi - b * HW
    y = pix // W
    x = pix - y * W
    ux, uy = up(b, y, x)
    for t in range(T):
        flows[t, b, 0, pix] = (sb[t][:, None] * ux).sum(axis=0) * scale
        flows[t, b, 1, pix] = (sb[t][:, None] * uy).sum(axis=0) * scale
    flows = flows.reshape(T, B, 2, H, W)

    # ---- k_cvx_bwd_centres, workgroups [0, nA): one thread per (sample, tile centre)
    gm = np.full((B * 576, plane), nan)
    writes = np.zeros((B * 576, plane), dtype=np.int64)
    ws_d, ws_w = np.full((B, 2 * d, n), nan), np.full((B, 9, n), nan)
    if B * n:
        b, i, y, x = centre_threads()
        gx = (sb.T[:, :, None] * G[b, :, i, 1].T[None]).sum(axis=1) * scale                   # [d, N]: sum_t basis[t][k] * gt.y
        gy = (sb.T[:, :, None] * G[b, :, i, 0].T[None]).sum(axis=1) * scale
        if mutant == 'xy_swapped':
            gx, gy = gy, gx
        wk, ch = softmax9(b, y, x)
        ws_d[b[None], np.arange(d)[:, None], i[None]] = gx
        ws_d[b[None], d + np.arange(d)[:, None], i[None]] = gy
        ws_w[b[None], np.arange(9)[:, None], i[None]] = wk
        cy, cx = y >> 3, x >> 3
        g9 = np.zeros((9, y.size))
        for k in range(9):
            _, _, _, use, cell = neighbour(k, cy, cx)
            pn = 8.0 * P[b[None], np.arange(2 * d)[:, None], cell[None]]
            g9[k] = np.where(use, (pn[:d] * gx).sum(axis=0) + (pn[d:] * gy).sum(axis=0), 0.0)
        dot = (wk * g9).sum(axis=0)
        rows = b[None] * 576 + np.arange(9)[:, None] * 64 + ch[None]
        cols = np.broadcast_to((cy * w + cx)[None], rows.shape)
        gm[rows, cols] = wk * (g9 - dot)
        np.add.at(writes, (rows, cols), 1)

    # ---- k_cvx_bwd_centres, workgroups [nA, ..): the zero fill, one workgroup per (plane, chunk of 1024), four elements a thread
    chunks = -(-plane // FILL_ELEMS)
    pl, chunk, th = (a.reshape(-1) for a in np.meshgrid(np.arange(B * 576), np.arange(chunks), np.arange(256), indexing='ij'))
    if mutant == 'fill_first_chunk_only':
        keep = chunk == 0
        pl, chunk, th = pl[keep], chunk[keep], th[keep]
    chn = pl % 576
    sy, sx = (chn >> 3) & 7, chn & 7
    uni = 8 % tile == 0 or mutant == 'fill_uni_always'
    plane_centre = _is_centre(sy, s, tile) & _is_centre(sx, s, tile)
    if uni and bool(plane_centre.any()):
        census.add('fill_uni_early_return')
    live = ~plane_centre if uni else np.ones_like(plane_centre)
    pl, chunk, th, sy, sx = pl[live], chunk[live], th[live], sy[live], sx[live]
    e0 = chunk * FILL_ELEMS + th * 4
    every = e0 + 3 < plane
    z, quad_centre = [], np.zeros_like(every)
    for q in range(4):
        e = e0 + q
        c = np.zeros_like(every)
        if not uni:
            cy = e // w
            cx = e - cy * w
            c = _is_centre(8 * cy + sy, s, tile) & _is_centre(8 * cx + sx, s, tile) & (e < plane)
        z.append((e < plane) & ~c)
        quad_centre |= c
        every = every & z[q]
    vec = every & ((base_offset + pl * plane + e0) % 4 == 0)
    wrote = z[0] | z[1] | z[2] | z[3]
    if bool(vec.any()):
        census.add('fill_float4_store')
    if bool((wrote & ~vec).any()):
        census.add('fill_scalar_store')
    if bool((wrote & (chunk > 0)).any()):
        census.add('fill_chunk_above_0')
    if not uni:
        census.update({'fill_per_element_quad_with_a_centre'} if bool(quad_centre.any()) else ())
        census.update({'fill_per_element_quad_without_a_centre'} if bool((wrote & ~quad_centre).any()) else ())
    for q in range(4):
        gm[pl[z[q]], e0[z[q]] + q] = 0.0                 # (a mutant's fill lands after the centres' stores)
        np.add.at(writes, (pl[z[q]], e0[z[q]] + q), 1)
    if mutant is None:                                    # the two roles write disjoint elements that together are the whole tensor
        assert bool((writes == 1).all()), (name, int((writes == 0).sum()), int((writes > 1).sum()))

    # ---- k_cvx_bwd_params: one thread per (cell, channel, sample); the nine cells whose centres see this one as neighbour k
    cell = np.arange(plane)
    cy, cx = cell // w, cell - (cell // w) * w
    acc = np.zeros((B, 2 * d, plane))
    for k in range(9):
        sign = 1 if mutant == 'gather_same_k' else -1
        qy, qx = cy + sign * (k // 3 - 1), cx + sign * (k % 3 - 1)
        y0, x0 = 8 * qy, 8 * qx
        ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w) & ~((y0 + 7 < s) | (x0 + 7 < s))
        iy_lo, ix_lo = np.where(y0 > s, (y0 - s + tile - 1) // tile, 0), np.where(x0 > s, (x0 - s + tile - 1) // tile, 0)
        iy_hi, ix_hi = np.minimum((y0 + 7 - s) // tile, nty - 1), np.minimum((x0 + 7 - s) // tile, ntx - 1)
        if mutant == 'gather_hi_unclipped':               # the upper ends not clipped to the cell's last row and column
            iy_hi, ix_hi = np.full_like(iy_hi, nty - 1), np.full_like(ix_hi, ntx - 1)
        cnt = np.where(ok, np.maximum(iy_hi - iy_lo + 1, 0) * np.maximum(ix_hi - ix_lo + 1, 0), 0)
        if k == 4:
            for v, tag in ((0, 0), (1, 1)):
                census.update({('centres_in_a_cell', tag)} if bool((cnt == v).any()) else ())
            census.update({('centres_in_a_cell', 'several')} if bool((cnt > 1).any()) else ())
        if bool((ok & (cnt == 0)).any()):
            census.add('gather_range_empty')
        if not n or not bool(cnt.any()):
            continue
        term = ws_w[:, None, k] * ws_d                                                        # [B, 2d, n]
        if mutant == 'gather_hi_unclipped':               # everything from (iy_lo, ix_lo) on: a suffix sum of the centre grid
            sfx = np.zeros((B, 2 * d, nty + 1, ntx + 1))
            sfx[:, :, :nty, :ntx] = term.reshape(B, 2 * d, nty, ntx)[:, :, ::-1, ::-1].cumsum(axis=2).cumsum(axis=3)[:, :, ::-1, ::-1]
            acc = acc + np.where(ok, sfx[:, :, np.clip(iy_lo, 0, nty), np.clip(ix_lo, 0, ntx)], 0.0)
            continue
        for a in range(int((iy_hi - iy_lo + 1)[ok].max())):
            for c in range(int((ix_hi - ix_lo + 1)[ok].max())):
                iy, ix = iy_lo + a, ix_lo + c
                take = ok & (iy <= iy_hi) & (ix <= ix_hi)
                acc = acc + np.where(take, term[:, :, np.clip(iy * ntx + ix, 0, n - 1)], 0.0)
    gp = (8.0 * acc).reshape(B, 2 * d, h, w)

    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()     # noqa: E731
    return types.SimpleNamespace(traj=f32(traj), flows=f32(flows), dflow=f32(ws_d), weights=f32(ws_w), grad_mask=f32(gm.reshape(B, 576, h, w)),
                                 grad_params=f32(gp), census=census)
