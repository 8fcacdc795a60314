"""Named cases of the event kernels (csrc/events.hip over csrc/ev_device.h: k_ev_bin -> k_iwe_accum forward, k_lut_accum backward in its
record and ordered variants, the global-atomic kernels k_splat_fwd_atomic / k_splat_bwd_atomic), their float64 reference, and the rule by which
every output element is compared with it.  A helper module (no fixtures): tests/test_event_cases_host.py checks the cases, the
reference and the comparator on the CPU (a float32 stand-in passes, nine mutants of it fail), tests/test_gpu_event_cases.py runs
the cases on the device.

The reference restates oracle.focus_oracle.warp_events / event_weights / bilinear_vote (reference focus.py:182-230,
event_image_converter.py:333-391) and their adjoint with respect to the LUT; it never calls the library.  DISCRETE DECISIONS are taken
in float32 exactly as the kernel takes them (`decisions`): the LUT cell it = int(bin), iy = floor(y / sp), ix = floor(x / sp) clamped
to the table (the documented deviation, ev_device.h:31-34; the division is mpc_div_sp, common.h:150-152: a multiplication by the exact
reciprocal for a power of two, an IEEE division otherwise), pos = fl32(lut + event) [43-44], dt = clamp(|t - t_ref|, 0, 1) and the
weight (1 - dt) * valid [48-49], the four strict border comparisons [53], floor(fl32(pos + 1e-6f)) [57], weight == 0 votes for nothing
[63], polarity block by row index < num_pos [events.hip:29, 253].  VALUES are float64 of those float32 inputs: fy = y - y0, the four tap
products, the weight, the position gradients gy = w ((1 - fx)(g10 - g00) + fx (g11 - g01)) and gx likewise, their sum per LUT cell, and
grad_out * (GCOEF * sum + add_term).

Every bound is a running error bound: gamma(k) = k u / (1 - k u), u = 2^-24, k = the fp32 roundings on the longest path of the kernel
to that value, applied to the absolute values.  The library is built with -ffp-contract=off (a contracted multiply-add rounds once
instead of twice, so contraction could only lower the counts).  The counts (lines of csrc/ev_device.h, or of
csrc/events.hip where it is named):

  N_TAP  9  a tap (1 - fy) (1 - fx) w: e[2] - t_ref (1) [48], 1 - dt (1), * valid (1) [49], fy = y - y0f (1) [58], 1 - fy (1), fx (1)
            [59], 1 - fx (1), the two products (2) [events.hip:337-340; 35-38].  (A first count of 8 had left out fx.)
  N_G    9  gy = w ((1 - fx)(g10 - g00) + fx (g11 - g01)): the weight's 3, fx (1), 1 - fx (1), g10 - g00 (1), the product (1), the
            addition (1), * w (1) [events.hip:419-420; 93-94]; gx the same through fy
  N_OUT  3  a cell of d/dLUT beyond its sum: the cast of the sum in mpc_from_fixed (1) [common.h:253-255], coef = GCOEF * grad_out (1)
            [events.hip:567], coef * sum (1) [570]; with add_term two more, grad_out * add (1) and the addition (1) [571]
  N_AT   2  a contribution of k_splat_bwd_atomic beyond gy: coef (1) [events.hip:58], coef * gy (1) [72]; the initial value grad_out *
            add_term (mpc_scale, one rounding) counts as one more contribution

  One rounding is NOT relative to the value it ends in: dt = |t - t_ref| is rounded relative to dt, and 1 - dt cancels, so the weight
  carries the ABSOLUTE error u dt |valid| whatever is left of it (a weight of 1e-6 from dt = 1 - 1e-6 may be off by 6 %).  Every tap
  and every gradient term therefore gets u dt |valid| times its position factors on top of the gamma term (E_DT below); the other
  subtractions have exact inputs where it matters (fy = y - y0f is exact by Sterbenz's lemma for every position whose taps can reach
  the image but y in (-0.5, 0), where fy >= 0.5 and the factor 1 - fy only meets taps outside the image).

  forward pixel     sum over taps (gamma(N_TAP) |tap64| + E_DT + 2^-30 [tap != 0]) + u |sum|: 2^-30 is the truncation of one
                    conversion (ev_to_fixed_small [events.hip:159-161], mpc_to_fixed [common.h:249-252]: both are the exact truncation of
                    tap * 2^30), u |sum| the cast in mpc_from_fixed.  mpc_event_splat_fwd_fixed: the same without the cast.
  backward cell     |coef| sum over events (gamma(N_G) |w| A + E_DT + 2^-30 [A > 0]), A = |1 - fx| (|g10| + |g00|) + |fx| (|g11| +
                    |g01|), then gamma(N_OUT) of the product and u each for grad_out * add_term and the addition.  mpc_to_fixed's
                    documented limit is |gy| < 2^31 (case large_adjoint stays below 2^30).
  atomic kernels    an fp32 sum in arbitrary order: gamma(n - 1 + N) times the sum of the absolute values of the n contributions
                    (N = N_TAP forward, N_G + N_AT backward), plus E_DT.

An element whose allowance is zero must be exactly zero (pixels no tap reaches, cells whose events have no tap inside the image and
no add_term).  Nothing is left out: positions and weights are the same bits on both sides, so the comparator has no "explained" set.
`compare` returns the largest |got - ref| / allowance with the index of that element and the events that touch it."""
import collections
import functools

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
Q30 = 2.0 ** -30
N_TAP, N_G, N_OUT, N_AT = 9, 9, 3, 2
N_ORACLE = 12      # oracle autograd per event: the weight's 3, fx, 1 - fx (2), three products per tap term (3), four terms added (3), one more for
                   # the second use of the fraction; its scatter / index_put order adds n - 1 (tests/test_event_cases_host.py)
T_REF = 0.41
GCOEF, GOUT = -1.37, 0.61          # neither 1, nor is their product exact in fp32
STANDIN_SR = 8                     # strip height of the stand-in's seam mutant (its own; the device's strips follow the CU count)
EV_STAGE, EV_CHUNK = 1152, 512     # csrc/tuning.h: records staged by a k_ev_bin workgroup, rows of one workgroup


def gamma(k):
    return k * U / (1.0 - k * U)


def _cdiv(a, b):
    return (a + b - 1) // b


class Case:
    """One named input: geometry, switches, events [B, M, 6] (y, x, t, p, bin, valid), LUT [B, nb, hq, wq, T, 2], adjoint image
    [B * T, P, H, W], add_term like the LUT, and `kind` [B, M]: index into `kinds`, the edge each row was placed for (0: padding)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def P(self):
        return 2 if self.split else 1

    @property
    def M(self):
        return self.ev.shape[1]

    def count(self, kind):
        return int((self.kind == self.kinds.index(kind)).sum()) if kind in self.kinds else 0

    def with_events(self, ev, kind=None):
        c = Case(**self.__dict__)
        c.ev = np.ascontiguousarray(ev, dtype=f32)
        c.kind = np.zeros(c.ev.shape[:2], dtype=np.int64) if kind is None else kind
        return c


# ---- discrete decisions, float32 (ev_device.h: warp_cell, warp_event_with) ----------------------------------------------------------
def div_sp(v, sp):
    return v * f32(1.0 / sp) if (sp & (sp - 1)) == 0 else v / f32(sp)


def cell_of(v, sp, n):
    return np.clip(np.floor(div_sp(np.asarray(v, dtype=f32), sp)), 0, n - 1).astype(np.int64)


def decisions(c, no_warp=False, unit_weight=False, mutant=None):
    """-> dict of [B, M, T] arrays: y, x, w (fp32), y0f, x0f (fp32 floors), live, pol, cell (flat index into [B, nb, hq, wq]), and the
    float64 weight w64 with the absolute error e_dt of its dt rounding.  `mutant`: the host stand-in's broken variants."""
    ev = c.ev
    B, M, _ = ev.shape
    T, H, W = c.T, c.H, c.W
    hq, wq = _cdiv(H, c.sp), _cdiv(W, c.sp)
    sh = (B, M, T)
    with np.errstate(all='ignore'):
        yo, xo = ev[..., 0], ev[..., 1]
        it = np.trunc(ev[..., 4]).astype(np.int64)
        if mutant != 'no_bin_clamp':
            it = np.clip(it, 0, c.nb - 1)
        iy, ix = cell_of(yo, c.sp, hq), cell_of(xo, c.sp, wq)
        cell = ((np.arange(B)[:, None] * c.nb + it) * hq + iy) * wq + ix
        cell = np.mod(cell, B * c.nb * hq * wq)            # (only the mutant leaves the table: it reads, and writes, a neighbour's slice)
        if no_warp:
            y, x = np.broadcast_to(yo[..., None], sh), np.broadcast_to(xo[..., None], sh)
        else:
            f = c.lut.reshape(-1, T, 2)[cell]                               # [B, M, T, 2]
            y, x = f[..., 0] + yo[..., None], f[..., 1] + xo[..., None]     # fp32 + fp32
        valid = np.ones_like(yo) if unit_weight else ev[..., 5]
        w = np.broadcast_to(valid[..., None], sh).astype(f32)
        v64 = np.broadcast_to(valid.astype(f64)[..., None], sh)
        w64, e_dt = v64.copy(), np.zeros(sh)
        if c.scale_dt:
            tr = np.asarray(c.t_ref, dtype=f32)[None, None, :]
            dt = np.abs(ev[..., 2][..., None] - tr)
            dt64 = np.abs(ev[..., 2].astype(f64)[..., None] - tr.astype(f64))
            if mutant != 'dt_unclamped':
                dt, dt64 = np.minimum(np.maximum(dt, f32(0)), f32(1)), np.clip(dt64, 0.0, 1.0)
            w = (f32(1) - dt) * w
            w64 = (1.0 - dt64) * v64
            e_dt = U * dt64 * np.abs(v64)
        if c.mask:
            low = (y <= 0) if mutant == 'mask_le' else (y < 0)
            oob = (y > f32(H)) | (x > f32(W)) | low | (x < 0)
            w = np.where(oob, f32(0), w)
        eps = f32(0) if mutant == 'floor_no_eps' else f32(1e-6)
        y0f, x0f = np.floor(y + eps), np.floor(x + eps)
        i = np.arange(M)[None, :, None]
        pol = ((i > c.num_pos) if mutant == 'pol_gt' else (i >= c.num_pos)) if c.split else np.zeros_like(i, dtype=bool)
        pol = np.broadcast_to(pol, sh).astype(np.int64)
        # a position whose taps can reach the image (the kernel clamps the floor to [-4, H + 4] before the int conversion [ev_device.h:61-62])
        near = (y0f >= -1) & (y0f <= H - 1) & (x0f >= -1) & (x0f <= W - 1)
    img = (np.arange(B)[:, None, None] * T + np.arange(T)[None, None, :]) * c.P + pol
    return dict(y=y, x=x, w=w, y0f=y0f, x0f=x0f, live=(w != 0), near=near, pol=pol, img=img, w64=w64, e_dt=e_dt,
                cell=np.broadcast_to(cell[..., None], sh), tr=np.broadcast_to(np.arange(T)[None, None, :], sh))


def _select(d, keys):
    """The live rows whose taps can reach the image, flattened; float32 positions as float64 with the floor taken off."""
    m = d['live'] & d['near']
    out = {k: d[k][m] for k in keys}
    out['row'] = np.broadcast_to(np.arange(m.shape[0] * m.shape[1]).reshape(m.shape[0], m.shape[1], 1), m.shape)[m]
    out['y0'], out['x0'] = d['y0f'][m].astype(np.int64), d['x0f'][m].astype(np.int64)
    out['fy'] = d['y'][m].astype(f64) - d['y0f'][m].astype(f64)
    out['fx'] = d['x'][m].astype(f64) - d['x0f'][m].astype(f64)
    return out


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def reference_fwd(c, no_warp=False, unit_weight=False):
    """-> dict: ref [B * T, P, H, W], allow (float image), allow_fixed (Q33.30 image), allow_atomic, n (taps per pixel), prov."""
    d = decisions(c, no_warp, unit_weight)
    s = _select(d, ('img', 'w64', 'e_dt'))
    H, W = c.H, c.W
    size = c.ev.shape[0] * c.T * c.P * H * W
    ref, mass, edt, nz = np.zeros(size), np.zeros(size), np.zeros(size), np.zeros(size)
    n = np.zeros(size, dtype=np.int64)
    pidx, prow = [], []
    g = 1.0 + gamma(N_TAP)
    for dy in (0, 1):
        for dx in (0, 1):
            ay, ax = (s['fy'] if dy else 1.0 - s['fy']), (s['fx'] if dx else 1.0 - s['fx'])
            yy, xx = s['y0'] + dy, s['x0'] + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = ((s['img'] * H + yy) * W + xx)[ok]
            tap = (ay * ax * s['w64'])[ok]
            np.add.at(ref, idx, tap)
            np.add.at(mass, idx, np.abs(tap))
            np.add.at(edt, idx, (np.abs(ay * ax) * s['e_dt'])[ok] * g)
            np.add.at(nz, idx, (tap != 0).astype(f64))
            np.add.at(n, idx, 1)
            pidx.append(idx)
            prow.append(s['row'][ok])
    shape = (c.ev.shape[0] * c.T, c.P, H, W)
    allow_fixed = gamma(N_TAP) * mass + edt + Q30 * nz
    allow = allow_fixed + U * (np.abs(ref) + allow_fixed)
    allow_atomic = gamma(np.maximum(n - 1, 0) + N_TAP) * mass + edt
    r = lambda a: a.reshape(shape)        # noqa: E731
    return dict(ref=r(ref), allow=r(allow), allow_fixed=r(allow_fixed), allow_atomic=r(allow_atomic), n=r(n), mass=r(mass),
                prov=(np.concatenate(pidx), np.concatenate(prow)))


def _adjoint_terms(c, s, gimg, dtype):
    """The four adjoint-image taps of every selected row (0 outside the image)."""
    H, W = c.H, c.W
    g = np.asarray(gimg, dtype=dtype).reshape(-1, H, W)

    def tap(dy, dx):
        yy, xx = s['y0'] + dy, s['x0'] + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok, g[s['img'], np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], dtype(0))
    return tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)


def reference_bwd(c, add=True, gcoef=GCOEF, gout=GOUT, extra=0):
    """-> dict: ref like the LUT, allow (tiled kernels), allow_atomic, n (live rows with a tap inside, per element), prov.
    `extra`: roundings per event on top of N_G (the oracle's autograd, N_ORACLE - N_G)."""
    d = decisions(c)
    s = _select(d, ('img', 'w64', 'e_dt', 'cell', 'tr'))
    g00, g10, g01, g11 = _adjoint_terms(c, s, c.gimg, f64)
    fy, fx, w = s['fy'], s['fx'], s['w64']
    gy = w * ((1 - fx) * (g10 - g00) + fx * (g11 - g01))
    gx = w * ((1 - fy) * (g01 - g00) + fy * (g11 - g10))
    Ay = np.abs(1 - fx) * (np.abs(g10) + np.abs(g00)) + np.abs(fx) * (np.abs(g11) + np.abs(g01))
    Ax = np.abs(1 - fy) * (np.abs(g01) + np.abs(g00)) + np.abs(fy) * (np.abs(g11) + np.abs(g10))
    size = c.lut.size
    S, E, ABS, EDT = np.zeros(size), np.zeros(size), np.zeros(size), np.zeros(size)
    n = np.zeros(size, dtype=np.int64)
    base = (s['cell'] * c.T + s['tr']) * 2
    kg = gamma(N_G + extra)
    for comp, val, A in ((0, gy, Ay), (1, gx, Ax)):
        idx = base + comp
        e_dt = s['e_dt'] * A * (1.0 + kg)
        np.add.at(S, idx, val)
        np.add.at(E, idx, kg * np.abs(w) * A + e_dt + Q30 * (A > 0))
        np.add.at(ABS, idx, np.abs(w) * A)
        np.add.at(EDT, idx, e_dt)
        np.add.at(n, idx, (A > 0).astype(np.int64))
    coef = float(f32(gcoef)) * float(f32(gout))
    v = coef * S
    Ev = abs(coef) * E + gamma(N_OUT) * abs(coef) * (np.abs(S) + E)
    if add:
        ga = float(f32(gout)) * c.add.astype(f64).reshape(-1)
        ref = v + ga
        allow = np.where((S == 0) & (E == 0), U * np.abs(ga), Ev + U * np.abs(ga) + U * (np.abs(v) + Ev + np.abs(ga) * (1 + U)))
        mass, contrib = abs(coef) * ABS + np.abs(ga), n + 1
    else:
        ref, allow, mass, contrib = v, Ev, abs(coef) * ABS, n
    allow_atomic = gamma(np.maximum(contrib - 1, 0) + N_G + extra + N_AT) * mass + abs(coef) * EDT
    r = lambda a: a.reshape(c.lut.shape)        # noqa: E731
    return dict(ref=r(ref), allow=r(allow), allow_atomic=r(allow_atomic), n=r(n),
                prov=(np.concatenate((base, base + 1)), np.concatenate((s['row'], s['row']))))


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'ratio index provenance')
RATIOS = {}          # (case, path) -> largest ratio seen


def compare(got, ref, allowance, case=None, prov=None):
    """Every element: |got - ref| <= allowance; where the allowance is 0 the two must be equal, and a non-finite value fails.
    -> Result(largest |got - ref| / allowance (inf for a failure at allowance 0), index of that element, the events touching it as
    'kind(sample, row)' strings)."""
    ref = np.asarray(ref, dtype=f64)
    got = np.asarray(got, dtype=f64).reshape(ref.shape)
    allowance = np.broadcast_to(np.asarray(allowance, dtype=f64), ref.shape)
    with np.errstate(all='ignore'):
        err = np.abs(got - ref)
        err = np.where(np.isfinite(err), err, np.inf)
        ratio = np.where(allowance > 0, err / np.where(allowance > 0, allowance, 1.0), np.where(err == 0, 0.0, np.inf))
    if ratio.size == 0:
        return Result(0.0, (), ())
    flat = int(np.argmax(ratio))
    index = tuple(int(i) for i in np.unravel_index(flat, ref.shape))
    names = ()
    if case is not None and prov is not None:
        rows = np.unique(prov[1][prov[0] == flat])[:12]
        names = tuple(f'{case.kinds[int(case.kind.reshape(-1)[r])]}({int(r) // case.M}, {int(r) % case.M})' for r in rows)
    return Result(float(ratio.reshape(-1)[flat]), index, names)


def check(label, path, got, ref, allowance, case=None, prov=None):
    """compare, print the figures, record the ratio, and fail with the provenance of the worst element."""
    r = compare(got, ref, allowance, case, prov)
    got = np.asarray(got, dtype=f64).reshape(np.shape(ref))
    print(f'{label} {path}: ratio {r.ratio:.3f} at {r.index}  max allowance {float(np.max(allowance)) if np.size(allowance) else 0.0:.3e}', flush=True)
    RATIOS[(label, path)] = max(RATIOS.get((label, path), 0.0), r.ratio)
    if not r.ratio <= 1.0:
        a = np.broadcast_to(np.asarray(allowance, dtype=f64), np.shape(ref))
        raise AssertionError(f'{label} {path}: element {r.index}: got {float(got[r.index])!r}, float64 {float(np.asarray(ref)[r.index])!r}, '
                             f'allowance {float(a[r.index]):.3e}, ratio {r.ratio:.3f}; touched by {", ".join(r.provenance) or "no event"}')
    return r.ratio


# ---- a float32 stand-in of the kernel arithmetic (CPU), with the mutants that must fail ---------------------------------------------
MUTANTS = ('seam_drop', 'mask_le', 'floor_no_eps', 'pol_gt', 'sat2', 'dt_unclamped', 'pair_swap', 'add_coef', 'no_bin_clamp')


def _to_fixed(v, mutant=None):
    """ev_to_fixed_small and mpc_to_fixed both give trunc(v * 2^30): v * 2^30 and v - trunc(v) are exact in fp32."""
    v = np.asarray(v, dtype=f64)
    if mutant == 'sat2':
        v = np.clip(v, -2.0, 2.0)
    return np.trunc(v * 2.0 ** 30).astype(np.int64)


def _select32(d):
    m = d['live'] & d['near']
    s = {k: d[k][m] for k in ('img', 'w', 'cell', 'tr')}
    s['y0'], s['x0'] = d['y0f'][m].astype(np.int64), d['x0f'][m].astype(np.int64)
    s['fy'], s['fx'] = d['y'][m] - d['y0f'][m], d['x'][m] - d['x0f'][m]          # fp32
    return s


def standin_fwd(c, no_warp=False, unit_weight=False, mutant=None, fixed=False):
    d = decisions(c, no_warp, unit_weight, mutant)
    s = _select32(d)
    H, W = c.H, c.W
    acc = np.zeros(c.ev.shape[0] * c.T * c.P * H * W, dtype=np.int64)
    one = f32(1)
    for dy in (0, 1):
        for dx in (0, 1):
            ay, ax = (s['fy'] if dy else one - s['fy']), (s['fx'] if dx else one - s['fx'])
            yy, xx = s['y0'] + dy, s['x0'] + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            if mutant == 'seam_drop' and dy:
                ok &= ~((yy % STANDIN_SR == 0) & (s['fy'] < f32(1e-3)))
            v = ay * ax * s['w']
            assert v.dtype == f32
            np.add.at(acc, ((s['img'] * H + yy) * W + xx)[ok], _to_fixed(v, mutant)[ok])
    acc = acc.reshape(c.ev.shape[0] * c.T, c.P, H, W)
    return acc if fixed else (acc.astype(f64) * Q30).astype(f32)


def standin_bwd(c, add=True, gcoef=GCOEF, gout=GOUT, mutant=None):
    d = decisions(c, mutant=mutant)
    s = _select32(d)
    if mutant == 'pair_swap':
        # record_grad at x0 = W - 1: the pair is loaded at column W - 2 and column x0 is its SECOND element
        s2 = dict(s)
        s2['x0'] = np.where(s['x0'] == c.W - 1, c.W - 2, s['x0'])
        g00, g10, _, _ = _adjoint_terms(c, s2, c.gimg, f32)
        _, _, g01, g11 = _adjoint_terms(c, s, c.gimg, f32)
    else:
        g00, g10, g01, g11 = _adjoint_terms(c, s, c.gimg, f32)
    one = f32(1)
    fy, fx, w = s['fy'], s['fx'], s['w']
    gy = w * ((one - fx) * (g10 - g00) + fx * (g11 - g01))
    gx = w * ((one - fy) * (g01 - g00) + fy * (g11 - g10))
    assert gy.dtype == f32
    acc = np.zeros(c.lut.size, dtype=np.int64)
    base = (s['cell'] * c.T + s['tr']) * 2
    np.add.at(acc, base, _to_fixed(gy))
    np.add.at(acc, base + 1, _to_fixed(gx))
    coef = f32(gcoef) * f32(gout)
    v = coef * (acc.astype(f64) * Q30).astype(f32)
    if add:
        v = v + (coef if mutant == 'add_coef' else f32(gout)) * c.add.reshape(-1)
    assert v.dtype == f32
    return v.reshape(c.lut.shape)


# ---- case construction ---------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, name, H, W, sp, nb, seed, T=1, B=2, split=True, scale_dt=True, mask=True, lut_scale=3.0, gimg_scale=1.0):
        self.name, self.H, self.W, self.sp, self.nb, self.T, self.B = name, H, W, sp, nb, T, B
        self.split, self.scale_dt, self.mask = split, scale_dt, mask
        self.hq, self.wq = _cdiv(H, sp), _cdiv(W, sp)
        self.rng = np.random.default_rng(seed)
        self.lut = (lut_scale * self.rng.standard_normal((B, nb, self.hq, self.wq, T, 2))).astype(f32)
        self.gimg = (gimg_scale * self.rng.standard_normal((B * T, 2 if split else 1, H, W))).astype(f32)
        self.add = self.rng.standard_normal(self.lut.shape).astype(f32)
        self.kinds = ['pad']
        self.rows = {(b, p): [] for b in range(B) for p in range(2)}

    def _kind(self, kind):
        if kind not in self.kinds:
            self.kinds.append(kind)
        return self.kinds.index(kind)

    def _where(self, b, pol):
        b = int(self.rng.integers(self.B)) if b is None else b
        pol = int(self.rng.integers(2)) if pol is None else pol
        return b, pol

    def _time(self, t, bin_):
        t = float(self.rng.uniform(0.05, 0.95)) if t is None else t
        bin_ = float(min(max(int(np.floor(t * self.nb)), 0), self.nb - 1)) if bin_ is None else bin_
        return t, bin_

    def own(self, kind, y, x, b=None, pol=None, t=None, bin_=None, valid=1.0):
        """A row with its OWN position given; the warp takes it where the LUT says."""
        b, pol = self._where(b, pol)
        t, bin_ = self._time(t, bin_)
        self.rows[(b, pol)].append((np.array([y, x, t, 1.0 - pol, bin_, valid], dtype=f32), self._kind(kind)))

    def warped(self, kind, ty=None, tx=None, b=None, pol=None, t=None, valid=1.0):
        """A row whose WARPED coordinate is exactly ty and / or tx (fp32): searched over the LUT cells for one whose flow takes a
        position of its own cell there, fl32(flow + position) == target.  A coordinate left open lands somewhere inside the image."""
        b, pol = self._where(b, pol)
        t, bin_ = self._time(t, None)
        F = self.lut[b, int(bin_), :, :, 0, :]
        oky, Ey = self._solve(F[..., 0], ty, self.H, self.hq, np.arange(self.hq)[:, None])
        okx, Ex = self._solve(F[..., 1], tx, self.W, self.wq, np.arange(self.wq)[None, :])
        cand = np.argwhere(oky & okx)
        assert len(cand) > 0, (self.name, kind, ty, tx)
        iy, ix = cand[int(self.rng.integers(len(cand)))]
        self.rows[(b, pol)].append((np.array([Ey[iy, ix], Ex[iy, ix], t, 1.0 - pol, bin_, valid], dtype=f32), self._kind(kind)))

    def _solve(self, Fc, target, size, ncell, grid):
        if target is None:               # an own position anywhere in each cell; the cell qualifies if its flow keeps the row inside
            E = (grid * self.sp + self.rng.uniform(0.0, self.sp, Fc.shape)).astype(f32)
            return (cell_of(E, self.sp, ncell) == grid) & (Fc + E >= 1) & (Fc + E <= size - 2), E
        tgt = f32(target)
        E = (tgt - Fc).astype(f32)
        return (cell_of(E, self.sp, ncell) == grid) & ((Fc + E) == tgt), E

    def filler(self, n, valid=(0.2, 1.2)):
        for _ in range(n):
            self.own('filler', self.rng.uniform(-0.5, self.H), self.rng.uniform(-0.5, self.W), valid=float(self.rng.uniform(*valid)))

    def finish(self, pad_inside=0.05, pad_end=(True, True), num_pos=None, t_ref=None):
        """Padding (all-zero) rows go inside and at the end of each polarity block; the blocks of the samples get equal lengths."""
        rng = self.rng
        blocks = {}
        for (b, p), rows in self.rows.items():
            order = rng.permutation(len(rows))
            rows = [rows[i] for i in order]
            n_in = int(np.ceil(pad_inside * len(rows))) if len(rows) >= 2 else 0
            for _ in range(n_in):
                rows.insert(int(rng.integers(1, len(rows))), (np.zeros(6, dtype=f32), 0))        # never first, never last
            blocks[(b, p)] = rows
        if not self.split and num_pos is None:
            for b in range(self.B):                 # one block: the rows meant for the second follow those of the first
                blocks[(b, 0)], blocks[(b, 1)] = blocks[(b, 0)] + blocks[(b, 1)], []
        lens = [max(len(blocks[(b, p)]) for b in range(self.B)) for p in range(2)]
        lens = [n + (3 if (pad_end[p] and n > 1) else 0) for p, n in enumerate(lens)]
        M = lens[0] + lens[1]
        ev, kind = np.zeros((self.B, M, 6), dtype=f32), np.zeros((self.B, M), dtype=np.int64)
        for (b, p), rows in blocks.items():
            o = p * lens[0]
            for i, (r, k) in enumerate(rows):
                ev[b, o + i], kind[b, o + i] = r, k
        npos = lens[0] if num_pos is None else num_pos
        T = self.T
        tr = np.array([T_REF], dtype=f32) if T == 1 else np.linspace(0, 1, T).astype(f32)
        return Case(name=self.name, H=self.H, W=self.W, sp=self.sp, nb=self.nb, T=T, B=self.B, split=self.split, scale_dt=self.scale_dt,
                    mask=self.mask, num_pos=npos if self.split else M, ev=ev, kind=kind, kinds=list(self.kinds), lut=self.lut,
                    gimg=self.gimg, add=self.add, t_ref=tr if t_ref is None else np.asarray(t_ref, dtype=f32))


FRACS = (0.0, 2.0 ** -20, 0.5, 1.0 - 2.0 ** -20)


def _rows_and_columns(name, mask, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed, mask=mask, scale_dt=mask)
    for rep in range(3):
        for r in range(-1, bd.H + 1):
            for fr in FRACS:
                bd.warped(f'row{"_seam" if fr == FRACS[1] else ""}{"_first" if r + fr == 0 else ""}{"_above" if r == -1 else ""}'
                          f'{"_last" if r == bd.H - 1 else ""}{"_H" if r + fr == bd.H else ""}', ty=r + fr)
        for q in range(-1, bd.W + 1):
            for fr in FRACS:
                bd.warped(f'col{"_left" if q == -1 else ""}{"_last" if q == bd.W - 1 else ""}{"_W" if q + fr == bd.W else ""}', tx=q + fr)
    bd.filler(200)
    return bd.finish()


def _below_integer(name, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed)
    for k in range(1, bd.H + 1):
        bd.warped('row_nextafter', ty=np.nextafter(f32(k), f32(-np.inf)))
        bd.warped('row_5e-7', ty=f32(k - 5e-7))
    for k in range(1, bd.W + 1):
        bd.warped('col_nextafter', tx=np.nextafter(f32(k), f32(-np.inf)))
        bd.warped('col_5e-7', tx=f32(k - 5e-7))
    bd.filler(60)
    return bd.finish()


def _weights(name, scale_dt, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed, scale_dt=scale_dt)
    t0 = float(f32(T_REF))
    ws = (1e-6, 1.5, float(np.nextafter(f32(1.5), f32(np.inf))), 1.9999, 2.5, -2.5, 1000.0, -1000.0, -0.7)
    for rep in range(12):
        for w in ws:
            # t == t_ref: dt = 0 and the fp32 weight after the time scaling IS the valid column
            bd.warped(f'w={w:g}', ty=float(bd.rng.integers(1, bd.H - 2)) + 0.25, t=t0, valid=w)
        bd.warped('dt>=1', ty=10.5, t=t0 + 1.0 + 2.0 ** -20)        # dropped, not a record
        bd.warped('dt=1.3', ty=20.5, t=t0 + 1.3)                    # dropped; a weight of -0.3 without the clamp
        bd.warped('dt=-1.3', ty=21.5, t=t0 - 1.3)
        bd.warped('dt~1', ty=30.5, t=t0 + 1.0 - 1e-6)               # 1 - dt ~ 1e-6: the absolute error of dt's rounding is 6 % of it
        bd.warped('dt~1', ty=31.5, t=t0 - 1.0 + 1e-6, valid=1.5)
    bd.filler(150, valid=(-3.7, 3.7))
    return bd.finish()


def _polarity(name, mode, seed):
    """mode: num_pos of 'np0' | 'np1' | 'npM1' | 'npM' | 'mid' (split on), or 'off' (one image per sample)."""
    split = mode != 'off'
    bd = _Builder(name, 48, 64, 4, 3, seed, split=split)
    last = bd.B - 1
    pols = {'np0': (1,), 'npM': (0,), 'np1': (1,), 'npM1': (0,), 'mid': (0, 1), 'off': (0, 1)}[mode]
    for i in range(300):
        # the same row (so the same warped position) with different weights in the two blocks: a record in the wrong image shows
        y, x, t = bd.rng.uniform(4, bd.H - 4), bd.rng.uniform(4, bd.W - 4), float(bd.rng.uniform(0.05, 0.95))
        for p in pols:
            bd.own('twin', y, x, b=last if mode in ('off', 'mid') or i % 2 else 0, pol=p, t=t, valid=1.0 if p == 0 else 0.37)
    if mode == 'np1':
        for b in range(bd.B):
            bd.warped('single', ty=7.25, b=b, pol=0, valid=0.9)
    if mode == 'npM1':
        for b in range(bd.B):
            bd.warped('single', ty=7.25, b=b, pol=1, valid=0.9)
    single = mode in ('np1', 'npM1')
    c = bd.finish(pad_end=(not single and mode != 'mid', not single))
    if mode in ('np1', 'npM1', 'mid'):
        # live rows at indices num_pos - 1 and num_pos in every sample that has rows at all
        c.kinds.append('edge')
        for b in range(c.B):
            for i in (c.num_pos - 1, c.num_pos):
                if c.kind[b].any() and c.kind[b, i] == 0:
                    c.ev[b, i] = np.array([20.3, 30.6, 0.5, 1.0, 1.0, 0.8], dtype=f32)
                    c.kind[b, i] = c.kinds.index('edge')
    return c


def _clamped_cells(name, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed)
    # the border cells' flows point inwards, so the rows that were clamped to them land inside the image
    bd.lut[:, :, 0, :, 0, 0] = 7.0 + bd.rng.uniform(0, 3, bd.lut[:, :, 0, :, 0, 0].shape).astype(f32)
    bd.lut[:, :, -1, :, 0, 0] = -9.0 - bd.rng.uniform(0, 3, bd.lut[:, :, -1, :, 0, 0].shape).astype(f32)
    bd.lut[:, :, :, 0, 0, 1] = 7.0 + bd.rng.uniform(0, 3, bd.lut[:, :, :, 0, 0, 1].shape).astype(f32)
    bd.lut[:, :, :, -1, 0, 1] = -9.0 - bd.rng.uniform(0, 3, bd.lut[:, :, :, -1, 0, 1].shape).astype(f32)
    r = bd.rng
    for _ in range(120):
        bd.own('y<0', r.uniform(-6, -0.01), r.uniform(8, bd.W - 8))
        bd.own('y>=H', r.uniform(bd.H, bd.H + 6), r.uniform(8, bd.W - 8))
        bd.own('x<0', r.uniform(8, bd.H - 8), r.uniform(-6, -0.01))
        bd.own('x>=W', r.uniform(8, bd.H - 8), r.uniform(bd.W, bd.W + 6))
        bd.own('bin<0', r.uniform(4, bd.H - 4), r.uniform(4, bd.W - 4), bin_=float(r.choice([-1.0, -2.5, -7.0])))
        bd.own('bin>=nb', r.uniform(4, bd.H - 4), r.uniform(4, bd.W - 4), bin_=float(r.choice([3.0, 3.5, 11.0])))
    bd.own('y<0', -0.01, 20.0)
    bd.own('y>=H', float(bd.H), 20.0)
    bd.own('x>=W', 20.0, float(bd.W))
    bd.filler(150)
    return bd.finish()


def _sp3(name, seed):
    bd = _Builder(name, 45, 63, 3, 3, seed)
    for rep in range(2):
        for k in range(bd.hq + 1):
            for kind, v in (('3k', f32(3 * k)), ('3k_below', np.nextafter(f32(3 * k), f32(-np.inf))), ('3k+2.9999', f32(3 * k + 2.9999))):
                bd.own('row_' + kind, v, bd.rng.uniform(0, bd.W))
        for k in range(bd.wq + 1):
            for kind, v in (('3k', f32(3 * k)), ('3k_below', np.nextafter(f32(3 * k), f32(-np.inf))), ('3k+2.9999', f32(3 * k + 2.9999))):
                bd.own('col_' + kind, bd.rng.uniform(0, bd.H), v)
    bd.filler(300)
    return bd.finish()


def _far_flows(name, mask, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed, mask=mask, scale_dt=False)
    far = (1e3, -1e3, 1e9, -1e9, 3e38, -3e38)
    k = 0
    for it in range(bd.nb):
        for iy in range(0, bd.hq, 2):                  # every second LUT row holds far cells; the rest of the table stays ordinary
            for ix in range(iy % 3, bd.wq, 3):
                comp = k % 3                           # far in y, in x, in both
                v = far[k % len(far)]
                if comp in (0, 2):
                    bd.lut[:, it, iy, ix, 0, 0] = v
                if comp in (1, 2):
                    bd.lut[:, it, iy, ix, 0, 1] = v
                for _ in range(3):
                    bd.own(f'far{v:g}', iy * 4 + bd.rng.uniform(0, 4), ix * 4 + bd.rng.uniform(0, 4), bin_=float(it),
                           t=(it + 0.5) / bd.nb)
                k += 1
    bd.filler(400)
    return bd.finish()


def _lut_seams(name, H, seed):
    bd = _Builder(name, H, 96, 1, 3, seed)
    r = bd.rng
    for rep in range(6):
        for iy in range(bd.hq):                        # every LUT row, in bins 0 and 2
            bd.own('lut_row', iy + r.uniform(0, 1), r.uniform(0, bd.W), t=float(r.choice([0.1, 0.9])))
    for _ in range(120):                               # bin 1 has rows in the first 8 LUT rows only: its other strips see no event
        bd.own('bin1_top', r.uniform(0, 8), r.uniform(0, bd.W), t=0.5)
    return bd.finish()


def _tiny_strip(name, seed):
    bd = _Builder(name, 48, 64, 16, 3, seed)
    r = bd.rng
    for it in range(bd.nb):                            # all the rows of a bin in ONE cell of the 3 x 4 table
        cy, cx = it % bd.hq, (it + 1) % bd.wq
        for _ in range(1100):
            bd.own(f'bin{it}_one_cell', cy * 16 + r.uniform(0, 16), cx * 16 + r.uniform(0, 16), t=(it + r.uniform(0.05, 0.95)) / bd.nb)
    return bd.finish()


def _large_adjoint(name, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed, gimg_scale=3000.0)
    np.clip(bd.gimg, -1e4, 1e4, out=bd.gimg)
    bd.gimg[:, :, ::7, ::5] = 1e4
    bd.filler(900, valid=(-50.0, 50.0))
    for _ in range(50):
        bd.own('w50', bd.rng.uniform(0, bd.H), bd.rng.uniform(0, bd.W), valid=50.0, t=float(f32(T_REF)))
    return bd.finish()


def _num_tref_3(name, seed):
    bd = _Builder(name, 48, 64, 4, 3, seed, T=3, split=False, scale_dt=False)
    for r in range(-1, bd.H + 1):
        bd.warped('row', ty=r + 0.5)
        bd.warped('row_seam', ty=r + 2.0 ** -20)
    bd.filler(900)
    return bd.finish()


# name: (builder, arguments) -- what each case exists for, and the host mutant(s) it catches (tests/test_event_cases_host.py)
CASES = {
    # every image row and column as y0 / x0 at fractions {0, 2^-20, 0.5, 1 - 2^-20}: taps straddle every possible strip seam, one tap
    # row / column inside at H - 1 / W - 1, y == 0, y == H, x == W on the strict comparisons.  Mutants: seam_drop, mask_le, pair_swap
    'rows_and_columns': (_rows_and_columns, (True, 11)),
    # the same with the border mask and the time scaling off: y0 = -1 and x0 = -1 vote with their one row / column inside (pair load of
    # record_grad at x0 = -1)
    'rows_and_columns_nomask': (_rows_and_columns, (False, 12)),
    # y = nextafter(k, -inf) and k - 5e-7: floor(y + 1e-6) lands on k, negative fraction, tap weights outside [0, 1].  Few rows per
    # image, so most of these stand alone in their pixels.  Mutant: floor_no_eps
    'below_integer': (_below_integer, (21,)),
    # the <= 1.5f switch between the two conversions of k_iwe_accum, weights that the time scaling leaves at exactly 0 or near it,
    # negative and large weights.  Mutants: sat2, dt_unclamped
    'weights': (_weights, (True, 31)),
    'weights_nodt': (_weights, (False, 32)),
    # live rows at num_pos - 1 and num_pos with num_pos in {0, 1, M - 1, M}, twins with different weights in the two blocks, records
    # in the last sample only.  Mutant: pol_gt
    'polarity_np0': (_polarity, ('np0', 41)),
    'polarity_np1': (_polarity, ('np1', 42)),
    'polarity_npM1': (_polarity, ('npM1', 43)),
    'polarity_npM': (_polarity, ('npM', 44)),
    'polarity_mid_last_sample': (_polarity, ('mid', 45)),
    'polarity_off_last_sample': (_polarity, ('off', 46)),
    # own position outside the image (y < 0, y >= H, x < 0, x >= W), bin below 0 and >= nb; the clamped cell's flow brings the row
    # back inside, and that cell receives its gradient.  Mutant: no_bin_clamp
    'clamped_cells': (_clamped_cells, (51,)),
    # the non-power-of-two division of mpc_div_sp: own positions at 3k, nextafter(3k, -inf), 3k + 2.9999
    'sp3': (_sp3, (61,)),
    # LUT entries of +-1e3, +-1e9, +-3e38: the +-4 clamp before the int conversion; nothing may be voted, exact zeros in d/dLUT
    'far_flows': (_far_flows, (False, 71)),
    'far_flows_masked': (_far_flows, (True, 72)),
    # 64 x 96 at sp 1: 6 144 cells, at least two LUT strips; rows on every LUT row, add_term random, strips without any event.
    # Mutant: add_coef
    'lut_seams': (_lut_seams, (64, 81)),
    # 80 x 96: with LUT strips of 64 KB (two of 40 rows = 3 840 cells) a strip has more cells than k_lut_accum prefetches of add_term
    'lut_seams_tall': (_lut_seams, (80, 82)),
    # 12 cells for 512 threads; thousands of integer atomics on one pair of accumulators
    'tiny_strip': (_tiny_strip, (91,)),
    # adjoint entries up to 1e4 with weights up to 50: the hi / lo split of mpc_to_fixed in the backward (documented limit |v| < 2^31)
    'large_adjoint': (_large_adjoint, (101,)),
    # T = 3 (time scaling and polarity split off): the global-atomic kernels, per-tr images and LUT slices
    'num_tref_3': (_num_tref_3, (111,)),
}

# case -> kinds of rows it must contain (the edge it is named for)
REQUIRED = {
    'rows_and_columns': ('row_seam', 'row_first', 'row_last', 'row_H', 'row_above', 'col_left', 'col_last', 'col_W', 'row', 'col'),
    'rows_and_columns_nomask': ('row_seam', 'row_above', 'row_seam_above', 'col_left', 'col_last'),
    'below_integer': ('row_nextafter', 'row_5e-7', 'col_nextafter', 'col_5e-7'),
    'weights': ('w=1e-06', 'w=1.5', 'w=1.9999', 'w=2.5', 'w=-2.5', 'w=1000', 'w=-1000', 'w=-0.7', 'dt>=1', 'dt=1.3', 'dt~1'),
    'weights_nodt': ('w=1e-06', 'w=1.5', 'w=2.5', 'w=-1000'),
    'polarity_np0': ('twin',), 'polarity_np1': ('twin', 'single'), 'polarity_npM1': ('twin', 'single'), 'polarity_npM': ('twin',),
    'polarity_mid_last_sample': ('twin',), 'polarity_off_last_sample': ('twin',),
    'clamped_cells': ('y<0', 'y>=H', 'x<0', 'x>=W', 'bin<0', 'bin>=nb'),
    'sp3': ('row_3k', 'row_3k_below', 'row_3k+2.9999', 'col_3k', 'col_3k_below', 'col_3k+2.9999'),
    'far_flows': ('far1000', 'far-1000', 'far1e+09', 'far-1e+09', 'far3e+38', 'far-3e+38'),
    'far_flows_masked': ('far1000', 'far-3e+38'),
    'lut_seams': ('lut_row', 'bin1_top'), 'lut_seams_tall': ('lut_row', 'bin1_top'),
    'tiny_strip': ('bin0_one_cell', 'bin1_one_cell', 'bin2_one_cell'),
    'large_adjoint': ('w50', 'filler'),
    'num_tref_3': ('row', 'row_seam'),
}
# mutant -> the cases that must catch it, and the direction ('fwd' | 'bwd')
CATCHES = {
    'seam_drop': ('fwd', ('rows_and_columns',)),
    'mask_le': ('fwd', ('rows_and_columns',)),
    'floor_no_eps': ('fwd', ('below_integer',)),
    'pol_gt': ('fwd', ('polarity_np0', 'polarity_np1', 'polarity_npM1', 'polarity_mid_last_sample')),
    'sat2': ('fwd', ('weights', 'weights_nodt')),
    'dt_unclamped': ('fwd', ('weights',)),
    'pair_swap': ('bwd', ('rows_and_columns', 'rows_and_columns_nomask')),
    'add_coef': ('bwd', ('lut_seams',)),
    'no_bin_clamp': ('bwd', ('clamped_cells',)),
}
T1_CASES = tuple(k for k in CASES if k != 'num_tref_3')
SPLAT_CASES = ('rows_and_columns', 'below_integer', 'weights')


@functools.lru_cache(maxsize=None)
def case(name):
    """-> Case (treat as read-only)."""
    fn, args = CASES[name]
    return fn(name, *args)


@functools.lru_cache(maxsize=None)
def expected_fwd(name):
    return reference_fwd(case(name))


@functools.lru_cache(maxsize=None)
def expected_bwd(name, add):
    return reference_bwd(case(name), add=add)


def splat_rows(name):
    """The warped positions and weights of a case as rows (y, x, -, -, -, weight) for ops.splat_events (MPC_F_NO_WARP, no mask, no
    time scaling): [B, M, 6] and the Case that describes them."""
    c = case(name)
    d = decisions(c)
    ev = np.zeros_like(c.ev)
    ev[..., 0], ev[..., 1], ev[..., 5] = d['y'][..., 0], d['x'][..., 0], c.ev[..., 5]
    s = c.with_events(ev, c.kind)
    s.split, s.scale_dt, s.mask, s.num_pos, s.nb = False, False, False, c.M, 1
    s.sp = max(c.H, c.W)
    return s
