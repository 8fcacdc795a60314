"""The IWE pyramid (UNPINNED extension: BASELINE.json's configs[2] names one, the reference has none) -- its DEFINITION in float64
and plain torch, and the cases the host and GPU tests of the fused pass (csrc/iwe_pyramid.hip) share.  Plain module imported by tests.

    level l + 1 = 2x2 average of the raw level l;  every level: 3x3 reflect blur (torchvision's sigma = 1 taps), Sobel with zero
    padding, val_l = mean over the level's own elements of |dx| + |dy| ('l1') or dx^2 + dy^2 ('l2');  focus = sum_l 1 / val_l."""
import contextlib
import functools

import torch
import torch.nn.functional as F

# ---- the pass alone: raw images [nimg, H, W], random non-negative fp32 ------------------------------------------------------
# (a) the coarsest level is 3x3, the limit; (b) level 1 is 40 x 232 and level 2 is 20 x 116: both cross the 56-column band edge,
# level 1 crosses the 32-row band edge (and the 16-row one the pass's own bands have); (c) narrower than a band; (d) the shape of
# (b) with a single non-zero pixel per image at a band corner: image 0 at level-0 (64, 112) = level-1 (32, 56), image 1 at
# level-0 (64, 224) = level-2 (16, 56).
CASES = {
    'a': dict(nimg=2, H=12, W=12, levels=3, seed=7),
    'b': dict(nimg=2, H=80, W=464, levels=3, seed=16),       # (seeds: the masked share of the 'l1' check, test_iwe_pyramid_host.py)
    'c': dict(nimg=3, H=16, W=8, levels=2, seed=9),
    'd': dict(nimg=2, H=80, W=464, levels=3, pixels=((64, 112), (64, 224))),
}
# the share of level-0 pixels grad_accounting.pyramid_near_zero_pixels masks for the 'l1' check must stay below this for the
# seeded cases (a one-pixel image is flat almost everywhere: (d) has no seed to choose and is exempt)
MASKED_SHARE_MAX = 0.02


@functools.lru_cache(maxsize=None)
def raw_images(name):
    c = CASES[name]
    if 'pixels' in c:
        raw = torch.zeros(c['nimg'], c['H'], c['W'])
        for i, (y, x) in enumerate(c['pixels']):
            raw[i, y, x] = 3.0
        return raw
    g = torch.Generator().manual_seed(c['seed'])
    # (event counts: mostly small, some zeros)
    return (torch.rand(c['nimg'], c['H'], c['W'], generator=g) * 4.0 - 0.5).clamp_(min=0.0)


def blur3(img):
    """[n, H, W] -> 3x3 blur, reflect padding, written out: taps exp(-x^2 / 2) / sum at x = -1, 0, 1, rows then columns summed."""
    e = torch.exp(torch.tensor(-0.5, dtype=img.dtype))
    a, c = e / (1 + 2 * e), 1 / (1 + 2 * e)
    p = F.pad(img[:, None], [1, 1, 1, 1], mode='reflect')[:, 0]
    h = a * p[:, :, :-2] + c * p[:, :, 1:-1] + a * p[:, :, 2:]
    return a * h[:, :-2] + c * h[:, 1:-1] + a * h[:, 2:]


def sobel(b):
    """[n, H, W] -> (dx, dy), zero padding, written out."""
    p = F.pad(b, [1, 1, 1, 1])
    tl, tc, tr = p[:, :-2, :-2], p[:, :-2, 1:-1], p[:, :-2, 2:]
    ml, mr = p[:, 1:-1, :-2], p[:, 1:-1, 2:]
    bl, bc, br = p[:, 2:, :-2], p[:, 2:, 1:-1], p[:, 2:, 2:]
    return (tr - tl) + 2 * (mr - ml) + (br - bl), (bl - tl) + 2 * (bc - tc) + (br - tr)


def level_value(raw_level, norm):
    dx, dy = sobel(blur3(raw_level))
    return (dx.square() + dy.square()).mean() if norm == 'l2' else (dx.abs() + dy.abs()).mean()


def definition64(raw, levels, norm):
    """raw [nimg, H, W] -> dict(vals [levels] float64, focus, grad: d focus / d raw [nimg, H, W] float64 by autograd)."""
    r = raw.double().clone().requires_grad_(True)
    vals, cur = [], r
    for _ in range(levels):
        vals.append(level_value(cur, norm))
        cur = F.avg_pool2d(cur[:, None], 2)[:, 0]
    focus = sum(1 / v for v in vals)
    (grad,) = torch.autograd.grad(focus, r)
    return dict(vals=torch.stack(vals).detach(), focus=focus.detach(), grad=grad)


def fold_ratios(level_scal):
    """r_l in float64 from the level table [levels, 8] of the pass (columns: include/mpcmax.h MPC_SCAL_*): 4^-l GCOEF_l / GCOEF_0,
    or 0 where a coefficient of level 0 .. l is 0, inf or NaN (a flat level passes nothing on); r_0 = 1."""
    c = level_scal[:, 4].double()
    ok = torch.isfinite(c) & (c != 0)
    out = [1.0]
    for l in range(1, len(c)):
        r = float(0.25 ** l * c[l] / c[0]) if bool(ok[:l + 1].all()) else 0.0
        out.append(r if abs(r) < float('inf') and r == r else 0.0)
    return out


def fold64(g_levels, level_scal):
    """The fold in float64 of the fp32 adjoint images g_levels[l] [nimg, H >> l, W >> l] (l = 0: grad_iwe before the pass):
    -> (sum_l r_l g_l[y >> l][x >> l], sum_l |r_l g_l| at every level-0 pixel)."""
    r = fold_ratios(level_scal)
    tot = torch.zeros(g_levels[0].shape, dtype=torch.float64)
    mag = torch.zeros_like(tot)
    for l, g in enumerate(g_levels):
        t = g.double().cpu().repeat_interleave(1 << l, -2).repeat_interleave(1 << l, -1) if r[l] != 0.0 else torch.zeros_like(tot)
        tot += r[l] * t
        mag += (r[l] * t).abs()
    return tot, mag


def fold_bound(mag, levels):
    """Per element: (2 L + 2) 2^-24 sum_l |r_l g_l| -- L - 1 adds, one product and one rounded ratio per term.  (The fold kernel
    rounds less often: one fused multiply-add per coarse level and the rounded ratio, 2 (L - 1) roundings, each at most 2^-24 of
    a partial sum that sum_l |r_l g_l| bounds; the bound of the stage-call chain's own roundings is the stated one.)"""
    return (2 * levels + 2) * 2.0 ** -24 * mag


# ---- the oracle chain of tests/test_gpu_pyramid.py::_oracle_pyramid for definitions that call O.make_iwes / O.contrast_value ---
@contextlib.contextmanager
def pyramid_objective(levels):
    """Inside: oracle.focus_oracle's make_iwes remembers the raw IWE it built and contrast_value answers with the pyramid's
    1 / sum_l (1 / val_l) on it, so that a definition which ends in `focus = 1 / O.contrast_value(iwes, ...)` -- the oracle's
    per-event basis warp, pe_curves_cases.definition -- states the pyramid of `levels` levels, gradient included."""
    from oracle import focus_oracle as O
    make_iwes, contrast_value = O.make_iwes, O.contrast_value
    kept = {}

    def make(*a, **k):
        iwes, raw = make_iwes(*a, **k)
        kept['raw'] = raw
        return iwes, raw

    def value(iwes, loss_type='gradient_magnitude', norm='l1'):
        cur = kept['raw'] if kept['raw'].dim() == 4 else kept['raw'][:, None]
        focus = 0.0
        for _ in range(levels):
            focus = focus + 1 / contrast_value(O.gaussian_blur3(cur), loss_type, norm)
            cur = F.avg_pool2d(cur, 2)
        return 1 / focus

    O.make_iwes, O.contrast_value = make, value
    try:
        yield
    finally:
        O.make_iwes, O.contrast_value = make_iwes, contrast_value
