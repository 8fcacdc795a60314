"""Named cases of the contrast and smoothness kernels (csrc/contrast.hip), their float64 reference, and the rule by which every
output element is compared with it.  A helper module (no fixtures): tests/test_contrast_cases_host.py checks the cases, the
reference and the comparator on the CPU (a float32 stand-in passes, five mutants of it fail), tests/test_gpu_contrast_cases.py
runs the cases on the device.

Every bound is a running error bound: gamma(k) = k u / (1 - k u), u = 2^-24, k = the fp32 roundings on the longest path of the
kernel to that value, times the same chain of operations applied to the absolute values of the inputs with the absolute values
of the stencil weights.  The counts (lines of csrc/contrast.hip; the library is built with -ffp-contract=off, and a contracted
multiply-add would round once instead of twice, so contraction could only lower them):

  N_TAP   4  a blur tap against its float64 value: the constant e (1), e + 1 (1), + e (1), the division (1)      [12-17]
  N_TAPB  5  a border weight of the blur adjoint, tap + tap (1 more)                                              [101-108]
  N_BLUR 14  hb = ka l + kc a + ka r: tap 4, product 1, two additions 2 = 7; B = ka hb2 + kc hb1 + ka hb0: 7 + 4 + 1 + 2
             [180, 183; k_contrast_fwd 56, 65]
  N_SOB  17  hd = B[c+1] - B[c-1] (15); dx = hd3 + 2 hd2 + hd1: the doubling is exact, two additions (17); dy = the same
             through vd = B1 - B3 [184, 189-191; k_contrast_fwd 85-86]
  N_L2T  36  dx dx + dy dy: 2 * 17 + 1 for a square, one addition                                                  [200; 87]
  N_L1T  18  |dx| + |dy|: one addition                                                                              [200; 87]
  N_ADJ  20  u -> adjoint image: hx = ux[c-1] - ux[c+1] (1), gx = hx2 + 2 hx3 + hx4 (2), g = gx + gy (1) = 4; the
             horizontal adjoint blur wx0 l + wx1 g + wx2 r: weight 5, product 1, two additions 2 = 8; the vertical one 8
             [204, 209-214, 218-221]
  N_L2G  37  u = 2 d is exact: 17 + 20
  N_VARG 16  variance adjoint, from blur - mean: row += w s (5 + 1 + 2 = 8), acc += wy row (8)                      [287-295]
  N_SD    3  smoothness Sobel on exact inputs: hd = r - l (1), dxx = hd2 + 2 hd1 + hd0 (2)                         [433, 438-440]
  N_ST    5  sqrt(d d + eps2) beyond the error of d: product 1, addition 1, eps2 = 1e-3f * 1e-3f against 1e-6 (3) -- five
             roundings under the root, so 2.5 -> 3, plus the hardware sqrt's 1 ulp = 2 u                             [410, 443-444]
  N_SV    8  v = d * rcp(sqrt(.)): the 3 above, sqrt 2 u, rcp 2 u, product 1                                       [445-446]
  N_SG    6  v -> grad_field: hx (1), hx1 + 2 hx2 + hx3 (2), + gy (1), gscale's own cast (1), the product (1)   [453, 457-462, 600]
  N_POOL  3  0.25 ((p0 + p1) + (p2 + p3)): three additions, the quarter is exact; backward r = 0.25 (cs / cb) (1),
             r * small (1), += (1)                                                                                  [704, 714-720]

Scalars are sums in fp64 on the device, so VAL's bound is the mean of the per-term bounds plus one fp32 rounding for the cast;
FOCUS = 1 / val and GCOEF = -k / val^2 take the exact difference 1 / (val - e) - 1 / val (resp. squared) of that bound, plus the
cast.  The smoothness gradient propagates the Sobel-response bound through d / sqrt(d^2 + eps^2) to first order with the float64
derivative eps^2 / s^3 at that cell, times 2 for the higher orders, plus N_SV u |v|.

l1 adjoint image: S = |Sobel| blur |raw| per pixel, tau = gamma(N_SOB) S.  A response is ambiguous where S > 0 and |d64| <= tau;
the reference takes u = sign(d64) with ambiguous entries 0, and every pixel must satisfy
|g_gpu - A u| <= |A| [ambiguous] + gamma(N_ADJ) |A| [S > 0], A = Blur^T Sobel^T.  Where no ambiguous response reaches, the
allowance is zero; at most L1_CAP of the pixels of an l1 case may have one."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import focus_oracle as O

U = 2.0 ** -24
N_TAP, N_TAPB, N_BLUR, N_SOB, N_L2T, N_L1T, N_ADJ, N_L2G, N_VARG = 4, 5, 14, 17, 36, 18, 20, 37, 16
N_SD, N_ST, N_SV, N_SG, N_POOL = 3, 5, 8, 6, 3
L1_CAP = 0.10
EPS = 1e-3
CF_TW, CT_H, CT_W, SM_W, SM_H, BAND_SWITCH = 56, 32, 64, 60, 16, 1536          # csrc/common.h, tuning.h, contrast.hip
SMOOTH_WEIGHT = float(np.float32(0.003))                                         # what the device sees of 0.003


def gamma(k):
    return k * U / (1.0 - k * U)


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- tilings restated (contrast.hip: mpc_contrast_fwd, smooth_band_rows; api.hip: mpc_layout) -----------------------------------
def contrast_band(H, W, nimg):
    """Rows per band of the marching contrast kernel."""
    return CT_H if _cdiv(W, CF_TW) * _cdiv(H, CT_H) * nimg >= BAND_SWITCH else CT_H // 2


def contrast_slots(H, W, nimg):
    """Entries of the partial-sum array (sized for 16-row bands)."""
    return _cdiv(W, CF_TW) * _cdiv(H, CT_H // 2) * nimg


def smooth_band(hq, wq, nimg, C):
    return SM_H if _cdiv(wq, SM_W) * _cdiv(hq, SM_H) * nimg * (C // 2) >= BAND_SWITCH else SM_H // 2


def smooth_blocks(hq, wq, nimg, C):
    return _cdiv(wq, SM_W) * _cdiv(hq, smooth_band(hq, wq, nimg, C)) * nimg * (C // 2)


# ---- the linear operators (any float dtype; images [n, H, W]) --------------------------------------------------------------
_KX = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)


def _conv(x, k):
    return F.conv2d(x[:, None], k.to(x.dtype)[None, None], padding=1)[:, 0]


def blur(x):
    return O.gaussian_blur3(x[:, None])[:, 0]


def sobel(b, absolute=False):
    if not absolute:
        dx, dy = O.sobel(b[:, None])
        return dx[:, 0], dy[:, 0]
    return _conv(b, _KX.abs()), _conv(b, _KX.t().abs())


def sobel_T(ux, uy, absolute=False):
    """Adjoint of the zero-padded Sobel pair: correlation with the flipped kernels."""
    kx, ky = _KX.flip(0, 1), _KX.t().flip(0, 1)
    if absolute:
        kx, ky = kx.abs(), ky.abs()
    return _conv(ux, kx) + _conv(uy, ky)


def blur_matrix(n, dtype=torch.float64):
    """M [n, n]: blurred coordinate q = sum_y M[q, y] raw[y], reflect padding of width 1."""
    k = O.blur_kernel_1d(dtype)
    M = torch.zeros(n, n, dtype=dtype)
    for q in range(n):
        for d in (-1, 0, 1):
            y = q + d
            y = -y if y < 0 else (2 * n - 2 - y if y >= n else y)
            M[q, y] += k[d + 1]
    return M


def blur_T(g, drop_fold_row=None):
    """Adjoint of the reflect-padded blur (its weights are non-negative: it is its own absolute version).  drop_fold_row: the
    host mutant that loses the fold of the ring below the last row into row H - 2."""
    H, W = g.shape[-2:]
    MH, MW = blur_matrix(H, g.dtype), blur_matrix(W, g.dtype)
    if drop_fold_row is not None:
        MH = MH.clone()
        MH[H - 1, H - 2] -= O.blur_kernel_1d(g.dtype)[0]
    return MH.t() @ g @ MW


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def image_reference(raw32, objective):
    """raw32 [n, H, W] fp32, objective 'l1' | 'l2' | 'variance' -> dict: blur / e_blur, val / e_val (before the cast), k (GCOEF =
    -k / val^2), gimg / e_gimg (unscaled adjoint image and its bound, the l1 allowance included), share (l1: pixels with a
    non-zero allowance) and allow (the allowance itself)."""
    raw = raw32.double()
    n, H, W = raw.shape
    b, ab = blur(raw), blur(raw.abs())
    r = dict(blur=b, e_blur=gamma(N_BLUR) * ab, share=0.0)
    if objective == 'variance':
        HW = H * W
        m = b.mean((-2, -1), keepdim=True)
        e_b = r['e_blur']
        var = ((b - m) ** 2).sum((-2, -1)) / (HW - 1)
        assert torch.allclose(var.mean(), O.contrast_value(b, 'variance'), rtol=1e-12, atol=0)
        e_var = ((2 * (b - m).abs() * e_b + e_b ** 2).sum((-2, -1)) + (HW + 4) * 2.0 ** -53 * (b ** 2).sum((-2, -1))) / (HW - 1)
        r['val'], r['e_val'] = float(var.mean()), float(e_var.mean())
        r['k'] = 2.0 / ((HW - 1) * n)
        e_m = e_b.mean((-2, -1), keepdim=True)
        e_m = e_m + U * (m.abs() + e_m)
        e_gb = e_b + e_m + U * ((b - m).abs() + e_b + e_m)
        r['gimg'] = blur_T(b - m)
        r['e_gimg'] = blur_T(e_gb) + gamma(N_VARG) * blur_T((b - m).abs() + e_gb)
        return r
    dx, dy = sobel(b)
    Sx, Sy = sobel(ab, absolute=True)
    N = raw.numel()
    r['k'] = 1.0 / N
    if objective == 'l2':
        val = O.contrast_value(b, 'gradient_magnitude', 'l2')
        e_term = gamma(N_L2T) * (Sx ** 2 + Sy ** 2)
        r['gimg'] = blur_T(sobel_T(2 * dx, 2 * dy))
        r['e_gimg'] = gamma(N_L2G) * blur_T(sobel_T(2 * Sx, 2 * Sy, absolute=True))
    else:
        val = O.contrast_value(b, 'gradient_magnitude', 'l1')
        e_term = gamma(N_L1T) * (Sx + Sy)
        tx, ty = gamma(N_SOB) * Sx, gamma(N_SOB) * Sy
        ax, ay = (Sx > 0) & (dx.abs() <= tx), (Sy > 0) & (dy.abs() <= ty)
        ux = torch.where(ax, torch.zeros_like(dx), torch.sign(dx))
        uy = torch.where(ay, torch.zeros_like(dy), torch.sign(dy))
        allow = blur_T(sobel_T(ax.double(), ay.double(), absolute=True))
        r['gimg'] = blur_T(sobel_T(ux, uy))
        r['e_gimg'] = allow + gamma(N_ADJ) * blur_T(sobel_T((Sx > 0).double(), (Sy > 0).double(), absolute=True))
        r['share'], r['allow'] = float((allow > 0).double().mean()), allow
        r['ambiguous'] = int(ax.sum() + ay.sum())
    r['val'] = float(val)
    r['e_val'] = float(e_term.mean()) + N * 2.0 ** -53 * float(val)
    return r


def smooth_reference(field32, weight=SMOOTH_WEIGHT):
    """field32 [nimg, hq, wq, C] fp32 -> dict: smooth / e_smooth (weight * smoothness, before the cast), gfield / e_gfield
    [nimg, hq, wq, C]."""
    f = field32.double().permute(0, 3, 1, 2)                          # [nimg, C, hq, wq]
    nimg, C, hq, wq = f.shape
    count = f.numel()
    fl = f.reshape(nimg * C, hq, wq)
    dx, dy = sobel(fl)
    bx, by = (gamma(N_SD) * v for v in sobel(fl.abs(), absolute=True))
    eps2 = EPS * EPS
    sx, sy = torch.sqrt(dx ** 2 + eps2), torch.sqrt(dy ** 2 + eps2)
    smooth = weight * float(O.smoothness(f, EPS))
    e_term = 2 * (dx.abs() / sx * bx + dy.abs() / sy * by) + gamma(N_ST) * (sx + sy)
    e_smooth = weight * (float(e_term.sum()) / count / 2.0 + count * 2.0 ** -53 * float(sx.mean() + sy.mean()))
    vx, vy = dx / sx, dy / sy
    e_vx = 2 * eps2 / sx ** 3 * bx + gamma(N_SV) * vx.abs()
    e_vy = 2 * eps2 / sy ** 3 * by + gamma(N_SV) * vy.abs()
    gs = weight / (2.0 * count)
    g = gs * sobel_T(vx, vy)
    e_g = gs * (sobel_T(e_vx, e_vy, absolute=True) + gamma(N_SG) * sobel_T(vx.abs(), vy.abs(), absolute=True))
    back = lambda t: t.reshape(nimg, C, hq, wq).permute(0, 2, 3, 1).contiguous()        # noqa: E731
    return dict(smooth=smooth, e_smooth=e_smooth, gfield=back(g), e_gfield=back(e_g), count=count)


def scalar_reference(img, sm=None):
    """-> {name: (value, bound)} of the five device scalars (mpc_finalize) from an image_reference and a smooth_reference."""
    v, e = img['val'], img['e_val']
    assert v > e >= 0, 'the objective of a case must stand clear of its own error bound'
    focus, e_f = 1.0 / v, e / (v * (v - e))
    k = img['k']
    gcoef, e_g = -k / (v * v), k * (1.0 / (v - e) ** 2 - 1.0 / (v * v))
    s, e_s = (sm['smooth'], sm['e_smooth']) if sm is not None else (0.0, 0.0)
    cast = lambda x, ex: ex + U * (abs(x) + ex)        # noqa: E731
    return dict(VAL=(v, cast(v, e)), FOCUS=(focus, cast(focus, e_f)), SMOOTH=(s, cast(s, e_s)),
                LOSS=(focus + s, cast(focus + s, e_f + e_s)), GCOEF=(gcoef, cast(gcoef, e_g)))


def pool_fwd_reference(x32):
    """[n, H, W] -> (2x2 mean over the floor(H / 2) x floor(W / 2) whole windows, its bound)."""
    x = x32.double()
    H2, W2 = x.shape[-2] // 2, x.shape[-1] // 2
    win = lambda t: t[:, :2 * H2, :2 * W2].reshape(-1, H2, 2, W2, 2)        # noqa: E731
    return 0.25 * win(x).sum((2, 4)), gamma(N_POOL) * 0.25 * win(x.abs()).sum((2, 4))


def pool_ratio(cs, cb):
    """The coefficient the backward applies (k_pool2_bwd_add): 0.25 cs / cb, or 0 where that is not a finite number."""
    with np.errstate(all='ignore'):
        ratio = np.float32(cs) / np.float32(cb)
    ok = np.float32(cb) != 0 and np.isfinite(ratio)
    return 0.25 * float(np.float64(np.float32(cs)) / np.float64(np.float32(cb))) if ok else 0.0


def pool_bwd_reference(small32, cs, cb, big32):
    """big[y][x] += r small[y / 2][x / 2] on the pooled part; the dropped odd last row / column keeps its value exactly (bound 0)."""
    big, small = big32.double(), small32.double()
    H2, W2 = small.shape[-2:]
    r = pool_ratio(cs, cb)
    up = small.repeat_interleave(2, -2).repeat_interleave(2, -1)
    out, e = big.clone(), torch.zeros_like(big)
    out[:, :2 * H2, :2 * W2] += r * up
    e[:, :2 * H2, :2 * W2] = gamma(N_POOL) * (big[:, :2 * H2, :2 * W2].abs() + abs(r) * up.abs()) if r != 0.0 else 0.0
    return out, e


# ---- the comparison -----------------------------------------------------------------------------------------------------------
RATIOS = {}          # output kind -> (largest error-to-bound ratio seen, label)


def compare(label, kind, got, ref, bound):
    """Every element: |got - ref| <= bound (0 where the bound is 0; a non-finite value fails).  Prints the figures, records the
    largest ratio under `kind`, raises an AssertionError naming the first bad element."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    got = torch.as_tensor(got).detach().cpu().double().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if not np.isfinite(ratio) or bool(bad.any()):
        ratio = float('inf') if bool(bad.any()) else ratio
    print(f'{label} {kind}: max |got - f64| {float(torch.nan_to_num(err, nan=float("inf")).max()) if err.numel() else 0.0:.3e}  '
          f'max bound {float(bound.max()) if bound.numel() else 0.0:.3e}  ratio {ratio:.3f}', flush=True)
    if ratio > RATIOS.get(kind, (-1.0, ''))[0]:
        RATIOS[kind] = (ratio, label)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0]) if ref.dim() else ()
        raise AssertionError(f'{label} {kind}: first bad element {idx}: got {float(got[idx])!r}, float64 {float(ref[idx])!r}, '
                             f'|difference| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e} ({int(bad.sum())} of {bad.numel()} bad)')
    return ratio


def compare_scalars(label, got, want, names=('VAL', 'FOCUS', 'SMOOTH', 'LOSS', 'GCOEF')):
    """got: {name: float} (the device's), want: scalar_reference()."""
    return max(compare(label, name, got[name], want[name][0], want[name][1]) for name in names)


# ---- inputs, seeded -----------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def img_dense(H, W, g):
    return torch.randn(H, W, generator=g)


def img_events(H, W, g):
    """Random bilinear 2 x 2 votes with random weights, about one per 60 pixels."""
    m = max(1, (H * W) // 60)
    x, y = torch.rand(m, generator=g).double() * (W - 1), torch.rand(m, generator=g).double() * (H - 1)
    w = 0.2 + torch.rand(m, generator=g).double()
    x0, y0 = x.floor().clamp(max=W - 2), y.floor().clamp(max=H - 2)
    fx, fy = x - x0, y - y0
    img = torch.zeros(H * W, dtype=torch.float64)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            img.put_(((y0 + dy) * W + x0 + dx).long(), w * wy * wx, accumulate=True)
    return img.reshape(H, W).float()


def img_isolated(H, W, g):
    img = torch.zeros(H, W)
    img[int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))] = 1.0
    return img


def img_constant(H, W, g):
    return torch.full((H, W), 0.75)


def img_offset(H, W, g):
    return 100.0 + torch.randn(H, W, generator=g)


def img_zero(H, W, g):
    return torch.zeros(H, W)


KINDS = dict(dense=img_dense, events=img_events, isolated=img_isolated, constant=img_constant, offset=img_offset, zero=img_zero)

# (H, W): every H of {3, 4, 15, 16, 17, 31, 32, 33, 47} (band edges at 16 and 32, two and three bands) at least twice, every W of
# {3, 4, 55, 56, 57, 59, 60, 61, 63, 64, 65, 113} (the 56- and 64-column tile edges; 113: three column groups) twice
IMG_SHAPES = ((3, 3), (4, 4), (3, 57), (4, 113), (15, 55), (15, 64), (16, 56), (16, 61), (17, 57), (17, 113), (31, 59), (31, 3),
              (32, 60), (32, 65), (33, 57), (33, 63), (47, 56), (47, 113), (33, 4), (16, 65), (17, 60), (32, 55), (15, 63), (47, 61))
# batch 'a': every objective; the isolated pixel joins it from 17 x 57 up (below, the l1 allowance would cover the image)
BATCH_A = ('dense', 'events', 'zero', 'events')
# batch 'b': l2, variance, blur and value only -- an isolated pixel and a constant image are ambiguous for l1 by construction
BATCH_B = ('isolated', 'constant', 'offset', 'dense', 'zero')
# (name, H, W, images): the band-height switch of the marching kernel at 33 x 57 (2 x 2 workgroups of 32 rows per image: 1536 at
# 384 images), and 1400 images: 8400 partial-sum slots (two trips of k_finalize) of which the 32-row bands use 5600
BIG_IMG = (('band32_384', 33, 57, 384), ('band16_383', 33, 57, 383), ('slots_1400', 33, 57, 1400))


def _img_name(H, W, batch):
    return f'{H}x{W}{batch}'


IMG_CASES = tuple(_img_name(H, W, b) for H, W in IMG_SHAPES for b in 'ab') + tuple(c[0] for c in BIG_IMG)
L1_CASES = tuple(_img_name(H, W, 'a') for H, W in IMG_SHAPES) + tuple(c[0] for c in BIG_IMG)
L2_CASES = IMG_CASES
VAR_CASES = tuple(_img_name(H, W, 'b') for H, W in IMG_SHAPES) + ('band16_383',)
FWD_CASES = tuple(_img_name(H, W, 'b') for H, W in IMG_SHAPES) + ('band32_384',)


@functools.lru_cache(maxsize=None)
def image_case(name):
    """-> raw [n, H, W] fp32 (treat as read-only)."""
    for big, H, W, n in BIG_IMG:
        if name == big:
            g = gen(7000 + n)
            raw = torch.randn(n, H, W, generator=g)
            for i in range(1, n, 3):
                raw[i] = img_events(H, W, g)
            raw[n // 2] = 0.0
            return raw
    H, W = (int(v) for v in name[:-1].split('x'))
    kinds = BATCH_A + (('isolated',) if H >= 17 and W >= 57 else ()) if name[-1] == 'a' else BATCH_B
    g = gen(1000 * H + W + (0 if name[-1] == 'a' else 500000))
    return torch.stack([KINDS[k](H, W, g) for k in kinds])


def lut_of(H, W, sp=4):
    return _cdiv(H, sp), _cdiv(W, sp)


@functools.lru_cache(maxsize=None)
def image_field(name):
    """The small dense LUT field [n, hq, wq, 2] (sp = 4) that goes with an image case, so that SMOOTH and LOSS are not trivial."""
    raw = image_case(name)
    n, H, W = raw.shape
    hq, wq = lut_of(H, W)
    return 2.0 * torch.randn(n, hq, wq, 2, generator=gen(31 * H + W + n))


@functools.lru_cache(maxsize=None)
def image_expected(name, objective):
    return image_reference(image_case(name), objective)


@functools.lru_cache(maxsize=None)
def field_expected(name):
    return smooth_reference(image_field(name))


# LUT fields: (hq, wq, C, nb, on_next) -- nimg = B nb or B (nb - 1) with B = 3; hq of {1, 2, 7, 8, 9, 15, 16, 17, 33}, wq of
# {1, 2, 3, 59, 60, 61, 62, 121}; C = 6 is num_tref = 3 (channel-pair stride 3)
FIELD_SHAPES = ((1, 1, 2, 3, False), (1, 60, 6, 3, True), (2, 3, 6, 3, False), (2, 121, 2, 3, True), (7, 59, 6, 2, False),
                (7, 2, 2, 3, False), (8, 60, 2, 3, False), (8, 61, 6, 3, True), (9, 61, 6, 3, False), (9, 3, 2, 2, True),
                (15, 62, 6, 3, False), (15, 1, 6, 3, True), (16, 121, 2, 3, False), (16, 59, 6, 3, True), (17, 61, 6, 3, False),
                (17, 1, 2, 3, False), (33, 2, 6, 3, True), (33, 121, 6, 2, False), (33, 62, 2, 3, True))
# (name, hq, wq, C, nimg): the band-height switch at 17 x 61 cells (2 x 2 workgroups of 16 rows per channel pair: 1536 at 384
# items), with both channel counts, and more than 8192 partial sums (2734 * 3 = 8202 workgroups of one band each)
BIG_FIELD = (('sband16_384', 17, 61, 2, 384), ('sband8_383', 17, 61, 2, 383), ('sband16_128x3', 17, 61, 6, 128),
             ('sband8_127x3', 17, 61, 6, 127), ('sparts_8202', 2, 3, 6, 2734))
FIELD_CASES = tuple(f'{hq}x{wq}c{C}{"n" if nx else "t"}{nb}' for hq, wq, C, nb, nx in FIELD_SHAPES) + tuple(c[0] for c in BIG_FIELD)


def field_geometry(name):
    """-> dict: hq, wq, C, nimg, and a shape the library accepts for it (B, nb, T, H, W, sp)."""
    for big, hq, wq, C, nimg in BIG_FIELD:
        if name == big:
            d = dict(hq=hq, wq=wq, C=C, nimg=nimg, B=nimg, nb=1)
            break
    else:
        hq, wq, C, nb, nx = FIELD_SHAPES[FIELD_CASES.index(name)]
        d = dict(hq=hq, wq=wq, C=C, nimg=3 * (nb - 1 if nx else nb), B=3, nb=nb)
    sp = 1 if min(d['hq'], d['wq']) >= 3 else 3                     # (images are at least 3 x 3)
    d.update(T=d['C'] // 2, sp=sp, H=d['hq'] * sp, W=d['wq'] * sp)
    return d


@functools.lru_cache(maxsize=None)
def field_case(name):
    """-> field [nimg, hq, wq, C] fp32: image 0 dense normal (a few pixels of flow), image 1 constant (only the zero-padded border
    responds), image 2 with Sobel responses around the Charbonnier epsilon, the rest dense at mixed scales."""
    d = field_geometry(name)
    g = gen(90000 + 1000 * d['hq'] + 7 * d['wq'] + d['C'] + d['nimg'])
    f = torch.randn(d['nimg'], d['hq'], d['wq'], d['C'], generator=g)
    f *= (10.0 ** torch.randint(-2, 2, (d['nimg'], 1, 1, 1), generator=g).float())
    f[0] = 3.0 * torch.randn(d['hq'], d['wq'], d['C'], generator=g)
    f[1] = -1.25
    f[2] = 2.0 + 3e-4 * torch.randn(d['hq'], d['wq'], d['C'], generator=g)
    return f


@functools.lru_cache(maxsize=None)
def smooth_expected(name):
    return smooth_reference(field_case(name))


POOL_SHAPES = ((2, 2), (3, 3), (5, 4), (4, 7), (33, 57), (47, 113))
POOL_COEFS = ((-0.5, -2.0), (0.0, -1.0), (-1.0, 0.0), (float('inf'), -1.0), (-1.0, float('inf')), (float('nan'), -1.0),
              (-1.0, float('nan')), (0.0, 0.0), (float('inf'), float('inf')), (-3e-3, -7e-5))
SCALE_COUNTS = (1, 255, 256, 257, 2048 * 256 + 1)


# ---- a float32 stand-in for the kernels (CPU; tests/test_contrast_cases_host.py), with the mutants that must fail --------------
def _partials(terms, band, stale=False):
    """Partial sums per (image, band of rows, group of 56 columns) in fp64 of fp32 terms, in the slots the marching kernel uses;
    the slots past the grid are cleared -- but for the `stale` mutant, which leaves the first of them with the value the finer
    tiling of the same data had written there."""
    n, H, W = terms.shape
    slots = np.zeros(contrast_slots(H, W, n))
    gx, gy = _cdiv(W, CF_TW), _cdiv(H, band)
    t = terms.double()
    for by in range(gy):
        for bx in range(gx):
            slots[(np.arange(n) * gy + by) * gx + bx] = t[:, by * band:(by + 1) * band, bx * CF_TW:(bx + 1) * CF_TW].sum((1, 2)).numpy()
    if stale and gx * gy * n < slots.size:
        e, fy, fh = gx * gy * n, _cdiv(H, CT_H // 2), CT_H // 2             # the first slot past the grid, in the finer tiling
        img, by, bx = e // (gx * fy), (e // gx) % fy, e % gx
        slots[e] = float(t[img, by * fh:(by + 1) * fh, bx * CF_TW:(bx + 1) * CF_TW].sum())
    return slots


def f32_contrast(raw32, objective, mutant=None):
    """-> dict blur, gimg (unscaled), VAL, FOCUS, GCOEF as float32 arithmetic gives them."""
    n, H, W = raw32.shape
    b = blur(raw32)
    if objective == 'variance':
        HW = H * W
        s1, s2 = b.double().sum((-2, -1)), (b.double() ** 2).sum((-2, -1))
        val = float(((s2 - s1 * s1 / HW) / (HW - 1)).mean())
        means = (s1 / HW).float()[:, None, None]
        gimg = blur_T(b - means)
        k = 2.0 / ((HW - 1) * n)
    else:
        dx, dy = sobel(b)
        if objective == 'l2':
            terms, ux, uy = dx * dx + dy * dy, 2 * dx, 2 * dy
        else:
            terms, ux, uy = dx.abs() + dy.abs(), torch.sign(dx), torch.sign(dy)
        val = float(_partials(terms, contrast_band(H, W, n), stale=mutant == 'stale_slot').sum()) / raw32.numel()
        gimg = blur_T(sobel_T(ux, uy), drop_fold_row=True if mutant == 'no_fold' else None)
        k = 1.0 / raw32.numel()
    out = dict(blur=b, gimg=gimg)
    if mutant == 'col56' and W > CF_TW:
        # the first column of the second group computed as if its left neighbour (a halo lane) held zero
        r2 = raw32.clone()
        r2[..., CF_TW - 1] = 0.0
        o2 = f32_contrast(r2, objective)
        for key in ('blur', 'gimg'):
            out[key] = out[key].clone()
            out[key][..., CF_TW] = o2[key][..., CF_TW]
    f = np.float32
    out.update(VAL=float(f(val)), FOCUS=float(f(1.0 / val)), GCOEF=float(f(-k / (val * val))), focus64=1.0 / val)
    return out


def f32_smooth(field32, weight=SMOOTH_WEIGHT, mutant=None):
    """-> dict SMOOTH, gfield [nimg, hq, wq, C] in float32 arithmetic.  Mutant 'pair_offset': channel pair 1 read where pair 0 is."""
    f = field32.permute(0, 3, 1, 2).contiguous()
    nimg, C, hq, wq = f.shape
    if mutant == 'pair_offset' and C > 2:
        f = f.clone()
        f[:, 2:4] = f[:, 0:2]
    fl = f.reshape(nimg * C, hq, wq)
    dx, dy = sobel(fl)
    eps2 = np.float32(1e-3) * np.float32(1e-3)
    sx, sy = torch.sqrt(dx * dx + eps2), torch.sqrt(dy * dy + eps2)
    count = f.numel()
    smooth = weight * ((float(sx.double().sum()) / count + float(sy.double().sum()) / count) / 2.0)
    gs = np.float32(weight / (2.0 * count))
    g = float(gs) * sobel_T(dx / sx, dy / sy)
    return dict(SMOOTH=float(np.float32(smooth)), smooth64=smooth, gfield=g.reshape(nimg, C, hq, wq).permute(0, 2, 3, 1).contiguous())


def f32_pool_fwd(x32):
    H2, W2 = x32.shape[-2] // 2, x32.shape[-1] // 2
    p = x32[:, :2 * H2, :2 * W2].reshape(-1, H2, 2, W2, 2)
    return 0.25 * ((p[:, :, 0, :, 0] + p[:, :, 0, :, 1]) + (p[:, :, 1, :, 0] + p[:, :, 1, :, 1]))


def f32_pool_bwd(small32, cs, cb, big32, mutant=None):
    """Mutant 'odd_row': an odd last row is not dropped, it receives the last pooled row."""
    H, W = big32.shape[-2:]
    H2, W2 = small32.shape[-2:]
    r = np.float32(pool_ratio(cs, cb))
    out = big32.clone()
    up = small32.repeat_interleave(2, -2).repeat_interleave(2, -1)
    out[:, :2 * H2, :2 * W2] += float(r) * up
    if mutant == 'odd_row' and H % 2:
        out[:, H - 1, :2 * W2] += float(r) * up[:, -1]
    return out
