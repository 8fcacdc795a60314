"""Named cases of the RAFT-spline correlation lookup (csrc/corr_lookup.hip), its float64 reference, and the rule by which every
element of every output is compared with it.  A helper module (no fixtures): tests/test_corr_cases_host.py checks the cases, the
reference and the comparator on the CPU (a float32 restatement of the kernels passes, nine mutants of it fail),
tests/test_gpu_corr_cases.py runs the cases on the device.

Reference.  The lookup's own formula in float64 (the one tools/gen_golden_corr.py states): entry e = (level l, slot k), target
t = level_target[l][k]; sample position coords[t] / 2^l + (j - r, i - r), x0 = floor, four taps, zero per tap outside the slice;
gradients by float64 autograd through it with floor detached (the one-sided derivative the kernel takes).  It never goes through
utils.corr._lookup_mirror, whose round trip through [-1, 1] moves an integer coordinate off the integer.  The documented clamp is
part of it: a scaled coordinate that is not finite or lies beyond +-CORR_COORD_LIMIT gives an all-zero window and no gradient.

Centre replay.  In Bezier mode the kernel forms the centre as fx = fx + basis[t][j] * p[j], j ascending, then (float)x + fx
(corr_centre, corr_lookup.hip:58-66).  `replay_centres` restates that in numpy float32, one rounding per operation, with the basis
the lookup itself uploads, and the float64 reference is evaluated AT these fp32 centres: cell, fractions and outputs are then
unambiguous and no element is left out of any comparison (the share of excluded elements is 0).  The distance between the replayed
and the float64 centre is checked on its own: gamma(2d + 1) (|x| + sum_j |basis| |p|) -- d products, d additions, the final one.

The rule, for every element: |device - float64| <= gamma(k) A, gamma(k) = k u / (1 - k u), u = 2^-24, A the same chain over absolute
values (the bilinear weights are non-negative), k the fp32 roundings on the longest path of the kernel to that value; where A is 0
the device value must be exactly 0.  The library is built with -ffp-contract=off (a contracted multiply-add would round once
instead of twice and could only lower the counts).  The counts, by line of csrc/corr_lookup.hip:

  the centre is an input (coords, or the replay above); c * 2^-l is exact [71-72]; fx = sx - floor(sx) is exact for sx >= 0 and for
  sx <= -0.5 [75] (see below for the rest)
  N_FWD   7  1 - fx, 1 - fy (1 each), w00 = (1 - fx)(1 - fy) (1): 3 on the longest weight; V * w (1); three additions (3)
             [175, 190; the lane-per-query kernel 100, 117]
  N_FILL  7  a window cell of grad_level, whole-slice route: the weight 3, g * w (1), v = v + ... four times of which the first
             adds to 0 exactly (3)                                                                   [422, 210-213; 465 / 450 copy]
  N_ACC   8  the accumulate route: the same cell gradient [270, 279-282], then prefill + v (1) [299], over |prefill| + sum |g| w
  N_CTR   5 + K K + levels   the centre gradient: 1 - fy (1) [335]; (V - V) (1) * ofy (1), the other product has one rounding
             less, their sum (1), go * (.) (1) = 5; ax = ax + ... K K times [352-353]; 2^-l * ax is exact [359-360]; the sum over
             the entries of a target, at most one per level [373-374]
  N_PAR   N_CTR + T + 1      grad_params: basis * grad centre (1), acc = acc + ... T times [393]

The inexact fraction.  For -0.5 < sx < 0 the difference sx - (-1) lies in (0.5, 1) and is rounded to a multiple of 2^-24: its
error is at most u / 2, and a tiny negative sx gives exactly 1.0f.  The output is bilinear in (fx, fy), so an axis in that interval
adds e S to the bound exactly, e = ex + ey + ex ey with ex, ey = u / 2 on such an axis and 0 elsewhere: for the forward S is the
sum of the four |taps| of that output; for a grad_level cell the sum of the up to four |cotangents| it gathers; for the centre
gradient 2^-l sum |g| (four |taps|) with the OTHER axis' e (d out / d fx depends on fy only).  First order in u: the gamma term is
taken at the exact fractions.

Nothing here is taken from the code under test, and no bound is changed after a run on the device."""
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
LIMIT = 1048576.0                                       # CORR_COORD_LIMIT
N_FWD, N_FILL, N_ACC = 7, 7, 8
CHUNK = 64                                              # queries per workgroup (forward, centre role, accumulate role)


def gamma(k):
    return k * U / (1.0 - k * U)


def n_centre(r, num_levels):
    return 5 + (2 * r + 1) ** 2 + num_levels


def n_params(r, num_levels, T):
    return n_centre(r, num_levels) + T + 1


def level_targets(nl):
    return [[t for t, v in enumerate(nl) if v >= l + 1] for l in range(max(nl))]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def basis_of(times, d, device='cpu'):
    """The [T, d] fp32 basis exactly as utils.CorrLookup uploads it."""
    from motionpriorcmax_amd.utils.basis import _device_basis
    return _device_basis('bernstein', [float(t) for t in times], (int(d),), torch.device(device), torch.float32)


def replay_centres(params, basis):
    """corr_centre in numpy float32: params [B, 2d, h, w], basis [T, d] -> [T, B, 2, h, w] fp32 tensor."""
    p = np.ascontiguousarray(params.detach().cpu().numpy(), dtype=np.float32)
    bm = np.ascontiguousarray(basis.detach().cpu().numpy(), dtype=np.float32)
    B, c2, h, w = p.shape
    T, d = bm.shape
    assert c2 == 2 * d
    xs = np.arange(w, dtype=np.float32)[None, None, :]
    ys = np.arange(h, dtype=np.float32)[None, :, None]
    out = np.empty((T, B, 2, h, w), dtype=np.float32)
    with np.errstate(all='ignore'):
        for t in range(T):
            fx, fy = np.zeros((B, h, w), dtype=np.float32), np.zeros((B, h, w), dtype=np.float32)
            for j in range(d):
                fx = fx + bm[t, j] * p[:, j]
                fy = fy + bm[t, j] * p[:, d + j]
            out[t, :, 0], out[t, :, 1] = xs + fx, ys + fy
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def centres64(params, basis):
    """The same centres in float64 (fp32 basis, as the fixtures' generator): [T, B, 2, h, w]."""
    B, c2, h, w = params.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    flows = torch.einsum('bcjhw,tj->tbchw', params.double().view(B, 2, c2 // 2, h, w), basis.double())
    return torch.stack((xs, ys), dim=0)[None, None] + flows


def replay_bound(params, basis):
    """gamma(2d + 1) (|x| + sum_j |basis| |p|): [T, B, 2, h, w]."""
    d = basis.shape[1]
    return gamma(2 * d + 1) * centres64(params.abs(), basis.abs())


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def reference(case, centres=None, want_levels=None):
    """-> namespace: out / e_out [B, E K K, h, w]; gc / e_gc [T, B, 2, h, w] (gradient of the centres, = grad_coords); gp / e_gp
    [B, 2d, h, w] (cases with params); gl / e_gl / inwin per level (None where not wanted) [n_l, B h w, 1, h_l, w_l]: the whole-slice
    route (`accum_reference` turns it into the accumulate route).
    `centres`: float64 [T, B, 2, h, w]; default the case's fp32 coordinates (the replayed centres of a Bezier case)."""
    c0 = (case.coords if centres is None else centres).double()
    T, B, _, h, w = c0.shape
    r, K, WN, hw = case.r, 2 * case.r + 1, 2 * case.r + 2, h * w
    L = len(case.levels)
    want = [True] * L if want_levels is None else list(want_levels)
    c = c0.clone().requires_grad_(True)
    g = case.g.double()
    vols = [lv.double().requires_grad_(True) if wt else lv.double() for lv, wt in zip(case.levels, want)]
    outs, e_outs = [], []
    A_gc, N_gc = torch.zeros_like(c0), torch.zeros_like(c0)
    A_gl, N_gl, inwin = [None] * L, [None] * L, [None] * L
    a = torch.arange(WN)
    ebase = 0
    for l, ts in enumerate(case.tix):
        n, (hl, wl) = len(ts), case.levels[l].shape[-2:]
        sl, NQ, inv = hl * wl, n * B * hw, 0.5 ** l
        s = c[ts] * inv                                                            # [n, B, 2, h, w]
        bad = (~torch.isfinite(s) | (s.abs() > LIMIT)).detach()
        s = torch.where(bad, torch.full_like(s, -LIMIT), s)
        sx, sy = s[:, :, 0].reshape(NQ), s[:, :, 1].reshape(NQ)
        x0, y0 = torch.floor(sx.detach()), torch.floor(sy.detach())
        fx, fy = (sx - x0)[:, None, None], (sy - y0)[:, None, None]
        yy, xx = y0.long()[:, None] - r + a, x0.long()[:, None] - r + a             # [NQ, WN]
        ok = (((yy >= 0) & (yy < hl))[:, :, None] & ((xx >= 0) & (xx < wl))[:, None, :])
        idx = (yy.clamp(0, hl - 1)[:, :, None] * wl + xx.clamp(0, wl - 1)[:, None, :]).reshape(NQ, WN * WN)
        W = vols[l].reshape(NQ, sl).gather(1, idx).reshape(NQ, WN, WN) * ok
        w00, w01, w10, w11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
        o = w00 * W[:, :K, :K] + w01 * W[:, :K, 1:] + w10 * W[:, 1:, :K] + w11 * W[:, 1:, 1:]

        def channels(v):                                                            # [NQ, K, K] -> [B, n K K, h, w]
            return v.reshape(n, B, h, w, K * K).permute(1, 0, 4, 2, 3).reshape(B, n * K * K, h, w)
        outs.append(channels(o))
        with torch.no_grad():
            Wa = W.abs()
            taps = (Wa[:, :K, :K], Wa[:, :K, 1:], Wa[:, 1:, :K], Wa[:, 1:, 1:])
            S4 = taps[0] + taps[1] + taps[2] + taps[3]
            ex = (((sx > -0.5) & (sx < 0)).double() * (U / 2))[:, None, None]
            ey = (((sy > -0.5) & (sy < 0)).double() * (U / 2))[:, None, None]
            exy = ex + ey + ex * ey
            e_outs.append(channels(gamma(N_FWD) * (w00 * taps[0] + w01 * taps[1] + w10 * taps[2] + w11 * taps[3]) + exy * S4))
            ga = g[:, ebase * K * K:(ebase + n) * K * K].reshape(B, n, K, K, h, w).permute(1, 0, 4, 5, 2, 3).reshape(NQ, K, K).abs()
            back = lambda v: v.sum((1, 2)).reshape(n, B, h, w)                      # noqa: E731
            A_gc[ts, :, 0] += inv * back(ga * ((taps[1] + taps[0]) * (1 - fy) + (taps[3] + taps[2]) * fy))
            A_gc[ts, :, 1] += inv * back(ga * ((taps[2] + taps[0]) * (1 - fx) + (taps[3] + taps[1]) * fx))
            N_gc[ts, :, 0] += inv * back(ey * ga * S4)
            N_gc[ts, :, 1] += inv * back(ex * ga * S4)
            if want[l]:
                cellA, cellG = torch.zeros(NQ, WN, WN, dtype=torch.float64), torch.zeros(NQ, WN, WN, dtype=torch.float64)
                for (i0, j0), wgt in (((0, 0), w00), ((0, 1), w01), ((1, 0), w10), ((1, 1), w11)):
                    cellA[:, i0:i0 + K, j0:j0 + K] += ga * wgt
                    cellG[:, i0:i0 + K, j0:j0 + K] += ga
                okf = ok.reshape(NQ, -1)
                shape = case.levels[l].shape
                A_gl[l] = torch.zeros(NQ, sl, dtype=torch.float64).scatter_add_(1, idx, cellA.reshape(NQ, -1) * okf).reshape(shape)
                inwin[l] = (torch.zeros(NQ, sl, dtype=torch.float64).scatter_add_(1, idx, okf.double()) > 0).reshape(shape)
                if bool((exy > 0).any()):
                    N_gl[l] = torch.zeros(NQ, sl, dtype=torch.float64).scatter_add_(1, idx, (exy * cellG).reshape(NQ, -1) * okf).reshape(shape)
        ebase += n
    out = torch.cat(outs, dim=1)
    wanted = [v for v, wt in zip(vols, want) if wt]
    grads = torch.autograd.grad(out, [c] + wanted, g)
    res = types.SimpleNamespace(out=out.detach(), e_out=torch.cat(e_outs, dim=1), gc=grads[0], inwin=inwin)
    kc = n_centre(r, L)
    res.e_gc = gamma(kc) * A_gc + N_gc
    it = iter(grads[1:])
    res.gl = [next(it) if wt else None for wt in want]
    res.A_gl = A_gl
    res.N_gl = [None if not wt else (N_gl[l] if N_gl[l] is not None else 0.0) for l, wt in enumerate(want)]
    res.e_gl = [gamma(N_FILL) * A_gl[l] + res.N_gl[l] if wt else None for l, wt in enumerate(want)]
    if case.params is not None:
        b64 = case.basis.double()
        d = b64.shape[1]
        fold = lambda m, v: torch.einsum('tj,tbahw->bajhw', m, v).reshape(B, 2 * d, h, w)        # noqa: E731
        res.gp = fold(b64, res.gc)
        res.e_gp = gamma(n_params(r, L, T)) * fold(b64.abs(), A_gc) + (1 + gamma(T + 1)) * fold(b64.abs(), N_gc)
    return res


def prefill(case):
    """Random finite contents of the shared gradient buffers before an accumulate launch (fp32, one per level)."""
    g = gen(977 + case.h * case.w)
    return [torch.randn(lv.shape, generator=g) for lv in case.levels]


def accum_reference(ref, pf):
    """MPC_CORR_F_GRAD_ACCUM over the buffers `pf`: -> (values, bounds) per level.  Inside a window prefill + gradient under
    gamma(N_ACC) (|prefill| + sum |g| w); everywhere else the kernel touches nothing: the prefill itself, bound 0."""
    vals, bounds = [], []
    for l, gl in enumerate(ref.gl):
        p64 = pf[l].detach().cpu().double().reshape(gl.shape)
        vals.append(p64 + gl)
        bounds.append(torch.where(ref.inwin[l], gamma(N_ACC) * (p64.abs() + ref.A_gl[l]) + ref.N_gl[l], torch.zeros_like(p64)))
    return vals, bounds


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def compare(label, kind, got, ref, bound, book=None):
    """Every element: |got - ref| <= bound (exactly ref where the bound is 0; a non-finite value fails).  Prints the figures, raises
    an AssertionError naming the first bad element.  book: a dict that collects, per output kind, [comparisons, elements, largest
    ratio, its label, the largest error and the largest bound of that comparison]."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    got = torch.as_tensor(got).detach().cpu().double().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    nbad = int(bad.sum())
    if nbad or not np.isfinite(ratio):
        ratio = float('inf')
    emax = float(torch.nan_to_num(err, nan=float('inf')).max()) if err.numel() else 0.0
    bmax = float(bound.max()) if bound.numel() else 0.0
    print(f'{label} {kind}: max |got - f64| {emax:.3e}  max bound {bmax:.3e}  ratio {ratio:.3f}  elements {ref.numel()}', flush=True)
    if book is not None:
        ent = book.setdefault(kind, [0, 0, -1.0, '', 0.0, 0.0])
        ent[0] += 1
        ent[1] += ref.numel()
        if ratio > ent[2]:
            ent[2:] = [ratio, label, emax, bmax]
    if nbad:
        idx = tuple(int(i) for i in torch.nonzero(bad)[0]) if ref.dim() else ()
        raise AssertionError(f'{label} {kind}: first bad element {idx}: got {float(got[idx])!r}, float64 {float(ref[idx])!r}, '
                             f'|difference| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e} ({nbad} of {bad.numel()} bad)')
    return ratio


def compare_all(label, ref, out=None, gc=None, gp=None, gl=None, book=None):
    """Whatever is given of: out, grad_coords, grad_params, the list of grad_level tensors (None entries are skipped)."""
    worst = 0.0
    if out is not None:
        worst = max(worst, compare(label, 'out', out, ref.out, ref.e_out, book))
    if gc is not None:
        worst = max(worst, compare(label, 'grad_coords', gc, ref.gc, ref.e_gc, book))
    if gp is not None:
        worst = max(worst, compare(label, 'grad_params', gp, ref.gp, ref.e_gp, book))
    for l, t in enumerate(gl or ()):
        if t is not None:
            worst = max(worst, compare(f'{label} level {l}', 'grad_level_fill', t, ref.gl[l], ref.e_gl[l], book))
    return worst


def compare_accum(label, ref, pf, gl, book=None):
    """The accumulate route: every element under its bound, and bit for bit the prefill outside every window."""
    vals, bounds = accum_reference(ref, pf)
    worst = 0.0
    for l, t in enumerate(gl):
        worst = max(worst, compare(f'{label} level {l}', 'grad_level_accum', t, vals[l], bounds[l], book))
        t = t.detach().cpu().reshape(pf[l].shape)
        assert torch.equal(t[~ref.inwin[l]].view(torch.int32), pf[l][~ref.inwin[l]].view(torch.int32)), (label, l)
    return worst


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _case(name, B, h, w, nl, r, d, seed, amp=3.0, coords=None, params=None, offset=False):
    """Random fp32 levels and cotangent; params drawn at `amp` unless given (d = 0: a case in coords mode only, `coords` given);
    coords of a Bezier case are its replayed centres."""
    g = gen(seed)
    nl = list(nl)
    tix = level_targets(nl)
    T, K = len(nl), 2 * r + 1
    levels = [torch.randn(len(ts), B * h * w, 1, h >> l, w >> l, generator=g) for l, ts in enumerate(tix)]
    assert all(lv.shape[-1] >= 2 and lv.shape[-2] >= 2 for lv in levels)
    cot = torch.randn(B, sum(nl) * K * K, h, w, generator=g)
    times = [(i + 1) / T for i in range(T)]
    basis = None
    if d:
        if params is None:
            params = torch.randn(B, 2 * d, h, w, generator=g) * amp
        params = params(g) if callable(params) else params
        basis = basis_of(times, d)
        coords = replay_centres(params, basis)
    else:
        coords = coords(g) if callable(coords) else coords
    assert tuple(coords.shape) == (T, B, 2, h, w) and coords.dtype == torch.float32
    return types.SimpleNamespace(name=name, B=B, h=h, w=w, nl=nl, tix=tix, T=T, r=r, d=d, times=times, levels=levels, g=cot,
                                 coords=coords, params=params, basis=basis, offset=offset, E=sum(nl))


def _grid(T, B, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    return torch.stack((xs, ys), dim=0)[None, None].repeat(T, B, 1, 1, 1)


LATTICE_R = 2


def _lattice_coords(T, B, h, w, r):
    """Multiples of 1/4 from -r - 2 up to (not including) w + r + 2 (h + r + 2): every integer of that range, each with its three
    quarters; every x value and every y value occurs, the two axes cycle at coprime strides."""
    X = [i + f for i in range(-r - 2, w + r + 2) for f in (0.0, 0.25, 0.5, 0.75)]
    Y = [i + f for i in range(-r - 2, h + r + 2) for f in (0.0, 0.25, 0.5, 0.75)]
    n = T * B * h * w
    k = torch.arange(n)
    cx = torch.tensor(X, dtype=torch.float32)[(k * 7) % len(X)]
    cy = torch.tensor(Y, dtype=torch.float32)[(k * 5 + 3) % len(Y)]
    return torch.stack((cx.reshape(T, B, h, w), cy.reshape(T, B, h, w)), dim=2)


def _neg_fraction_coords(T, B, h, w):
    def make(g):
        c = _grid(T, B, h, w) * 0.5 + torch.rand(T, B, 2, h, w, generator=g)                     # anywhere on the grid
        neg = -2.0 * torch.rand(T, B, 2, h, w, generator=g).clamp(2.0 ** -20, 1 - 2.0 ** -20)  # (-2, 0): (-1, 0) at level 1
        pick = torch.rand(T, B, 2, h, w, generator=g) < 0.6
        c = torch.where(pick, neg, c)
        special = [-2.0 ** -30, -2.0 ** -25, -0.25, -0.75, -0.5, -1.0 + 2.0 ** -24, -0.5 + 2.0 ** -25, -2.0 ** -24]
        assert T == 1 and B == 1
        for i, v in enumerate(special):                                                          # x from pixel 0 on, y from pixel 3 on
            c[0, 0, 0].view(-1)[i] = v
            c[0, 0, 1].view(-1)[i + 3] = v
        return c
    return make


NONFINITE = (float('nan'), float('inf'), float('-inf'), 1e30, -1e30, 2.0 ** 20, -2.0 ** 20)
_BAD_PIX = ((6, 8), (2, 5), (3, 3), (7, 4), (5, 1), (1, 2), (4, 7))                  # (y, x) on the 8 x 10 grid: both chunks of 64


def _nonfinite_coords(g):
    c = _grid(2, 1, 8, 10) + torch.randn(2, 1, 2, 8, 10, generator=g) * 2.0
    for i, ((y, x), v) in enumerate(zip(_BAD_PIX, NONFINITE)):
        c[i % 2, 0, (i // 2) % 2, y, x] = v
    return c


def _nonfinite_params(g):
    p = torch.randn(1, 6, 8, 10, generator=g) * 2.0
    for (y, x), v, ch in zip(_BAD_PIX, NONFINITE, (0, 4, 2, 5, 1, 0, 3)):
        p[0, ch, y, x] = v
    return p


RAGGED = [1, 3, 2, 1, 3, 2, 1, 3, 2, 1, 3, 2, 1, 3, 2, 1]

_SPECS = dict(
    # the first lookup of a forward: control points zero, integer coordinates at level 0, halves and quarters above
    zero_params=lambda: _case('zero_params', 1, 8, 10, [3, 2], 2, 3, 11, params=torch.zeros(1, 6, 8, 10)),
    lattice=lambda: _case('lattice', 2, 6, 7, [2, 2], LATTICE_R, 0, 12, coords=_lattice_coords(2, 2, 6, 7, LATTICE_R)),
    neg_fraction=lambda: _case('neg_fraction', 1, 4, 5, [2], 2, 0, 13, coords=_neg_fraction_coords(1, 1, 4, 5)),
    # one per radius: h w = 63, 64, 65, 130 (below, at and past a chunk of 64; B h w = 390 is no multiple of 4)
    r1=lambda: _case('r1', 1, 7, 9, [2, 1], 1, 2, 21),
    r2=lambda: _case('r2', 2, 8, 8, [3, 1], 2, 3, 22),
    r3=lambda: _case('r3', 1, 5, 13, [1, 2], 3, 4, 23),
    r4=lambda: _case('r4', 3, 10, 13, [2, 3], 4, 5, 24),
    limits_targets=lambda: _case('limits_targets', 1, 8, 9, RAGGED, 1, 16, 31),
    limits_full=lambda: _case('limits_full', 1, 8, 9, [3] * 16, 2, 16, 32),
    d1=lambda: _case('d1', 1, 6, 8, [2, 1], 4, 1, 33),
    six_levels=lambda: _case('six_levels', 1, 64, 64, [6], 1, 2, 34, amp=8.0),
    nonfinite=lambda: _case('nonfinite', 1, 8, 10, [2, 1], 2, 0, 41, coords=_nonfinite_coords),
    nonfinite_bezier=lambda: _case('nonfinite_bezier', 1, 8, 10, [2, 1], 2, 3, 42, params=_nonfinite_params),
    offset_views=lambda: _case('offset_views', 1, 8, 8, [2, 2], 3, 2, 51, offset=True),
)
CASES = tuple(_SPECS)
BEZIER_CASES = ('zero_params', 'r1', 'r2', 'r3', 'r4', 'limits_targets', 'limits_full', 'd1', 'six_levels', 'nonfinite_bezier', 'offset_views')
GUARD_CASES = ('r1', 'r2', 'r3', 'r4', 'offset_views')


@functools.lru_cache(maxsize=None)
def case(name):
    """Treat as read-only."""
    return _SPECS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(case(name))


def scaled_cells(cs, l):
    """x0, y0 (long, [T, B, h, w]) of the case's coordinates at level l; a clamped / non-finite one sits at -2^20."""
    s = cs.coords.double() * 0.5 ** l
    s = torch.where(~torch.isfinite(s) | (s.abs() > LIMIT), torch.full_like(s, -LIMIT), s)
    return torch.floor(s[:, :, 0]).long(), torch.floor(s[:, :, 1]).long()


def fractions32(cs, l):
    """The fp32 fractions the kernel forms at level l (corr_split): [T, B, 2, h, w]."""
    s = cs.coords * np.float32(0.5 ** l)
    s = torch.where(torch.isnan(s), torch.full_like(s, -LIMIT), s).clamp(-LIMIT, LIMIT)
    return s - torch.floor(s)


# ---- a float32 restatement of the kernels' expressions (CPU; tests/test_corr_cases_host.py), with the mutants that must fail -----
MUTANTS = ('trunc', 'round', 'edge_clamp', 'swap_w01_w10', 'origin', 'no_level_scale', 'target_major', 'slot_as_target', 'unwritten_cell')


def f32_lookup(cs, bezier=False, mutant=None, prefill=None):
    """-> namespace out, gc, gp (bezier), gl: torch float32 on the CPU, one rounding per operation, in the kernels' order.  The
    whole-slice route starts from NaN (what torch.empty may hold) and writes every element; with `prefill` the accumulate route."""
    f32 = torch.float32
    c = replay_centres(cs.params, cs.basis) if bezier else cs.coords
    T, B, _, h, w = c.shape
    r, K, WN, hw = cs.r, 2 * cs.r + 1, 2 * cs.r + 2, h * w
    a = torch.arange(WN)
    entries, ge, gl = [], {}, []
    ebase = 0
    for l, ts in enumerate(cs.tix):
        n, (hl, wl) = len(ts), cs.levels[l].shape[-2:]
        sl, NQ = hl * wl, n * B * hw
        inv = np.float32(0.5 ** l)
        used = list(range(n)) if (mutant == 'slot_as_target' and l > 0) else ts
        s = c[used] * inv
        s = torch.where(torch.isnan(s), torch.full_like(s, -LIMIT), s).clamp(-LIMIT, LIMIT)
        fl = torch.trunc(s) if mutant == 'trunc' else torch.floor(s + 0.5) if mutant == 'round' else torch.floor(s)
        fr = s - fl
        x0, y0 = fl[:, :, 0].reshape(NQ).long(), fl[:, :, 1].reshape(NQ).long()
        fx, fy = fr[:, :, 0].reshape(NQ, 1, 1), fr[:, :, 1].reshape(NQ, 1, 1)
        org = r - 1 if mutant == 'origin' else r
        yy, xx = y0[:, None] - org + a, x0[:, None] - org + a
        ok = (((yy >= 0) & (yy < hl))[:, :, None] & ((xx >= 0) & (xx < wl))[:, None, :])
        idx = (yy.clamp(0, hl - 1)[:, :, None] * wl + xx.clamp(0, wl - 1)[:, None, :]).reshape(NQ, WN * WN)
        W = cs.levels[l].reshape(NQ, sl).gather(1, idx).reshape(NQ, WN, WN)
        if mutant != 'edge_clamp':
            W = W * ok
        ofx, ofy = 1 - fx, 1 - fy
        w00, w01, w10, w11 = ofx * ofy, fx * ofy, ofx * fy, fx * fy
        if mutant == 'swap_w01_w10':
            w01, w10 = w10, w01
        o = ((W[:, :K, :K] * w00 + W[:, :K, 1:] * w01) + W[:, 1:, :K] * w10) + W[:, 1:, 1:] * w11
        assert o.dtype == f32
        o = o.reshape(n, B, h, w, K * K).permute(0, 1, 4, 2, 3)                      # [n, B, K K, h, w]
        g = cs.g[:, ebase * K * K:(ebase + n) * K * K].reshape(B, n, K, K, h, w).permute(1, 0, 4, 5, 2, 3).reshape(NQ, K, K)
        ax, ay = torch.zeros(NQ, dtype=f32), torch.zeros(NQ, dtype=f32)
        fx1, fy1, ofx1, ofy1 = fx.reshape(NQ), fy.reshape(NQ), ofx.reshape(NQ), ofy.reshape(NQ)
        for i in range(K):
            prev, cur = W[:, i], W[:, i + 1]
            for j in range(K):
                go = g[:, i, j]
                ax = ax + go * ((prev[:, j + 1] - prev[:, j]) * ofy1 + (cur[:, j + 1] - cur[:, j]) * fy1)
                ay = ay + go * ((cur[:, j] - prev[:, j]) * ofx1 + (cur[:, j + 1] - prev[:, j + 1]) * fx1)
        if mutant != 'no_level_scale':
            ax, ay = inv * ax, inv * ay
        for k in range(n):
            entries.append((l, ts[k], o[k]))
            ge[(l, ts[k])] = (ax.reshape(n, B, h, w)[k], ay.reshape(n, B, h, w)[k])
        v = torch.zeros(NQ, WN, WN, dtype=f32)
        for (i0, j0), wgt in (((0, 0), w00), ((0, 1), w01), ((1, 0), w10), ((1, 1), w11)):
            v[:, i0:i0 + K, j0:j0 + K] = v[:, i0:i0 + K, j0:j0 + K] + g * wgt
        okf = ok.reshape(NQ, -1)
        cell = torch.zeros(NQ, sl, dtype=f32).scatter_add_(1, idx, v.reshape(NQ, -1) * okf)          # (one non-zero term per element)
        if prefill is None:
            buf = torch.full((NQ, sl), float('nan'))
            buf[:] = cell                                                                # every element of the slice is written
        else:
            buf = prefill[l].reshape(NQ, sl).clone()
            hit = torch.zeros(NQ, sl, dtype=f32).scatter_add_(1, idx, okf.float()) > 0
            buf[hit] = buf[hit] + cell[hit]
        if mutant == 'unwritten_cell' and l == 0:
            q = int(torch.nonzero(okf.any(1))[0])
            buf[q, int(idx[q][okf[q]][0])] = float('nan')
        gl.append(buf.reshape(cs.levels[l].shape))
        ebase += n
    if mutant == 'target_major':
        entries.sort(key=lambda e: (e[1], e[0]))
    out = torch.cat([e[2] for e in entries], dim=1).contiguous()
    gc = torch.zeros(T, B, 2, h, w, dtype=f32)
    for t in range(T):
        for l, ts in enumerate(cs.tix):
            if t in ts:
                gc[t, :, 0] = gc[t, :, 0] + ge[(l, t)][0]
                gc[t, :, 1] = gc[t, :, 1] + ge[(l, t)][1]
    res = types.SimpleNamespace(out=out, gc=gc, gl=gl, gp=None)
    if bezier:
        d = cs.d
        gp = torch.zeros(B, 2, d, h, w, dtype=f32)
        for j in range(d):
            for t in range(T):
                gp[:, :, j] = gp[:, :, j] + cs.basis[t, j] * gc[t]
        res.gp = gp.reshape(B, 2 * d, h, w)
    return res
