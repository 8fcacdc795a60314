"""The cubic B-spline kind of FocusLoss.calc_per_event_curves (curve_type='BSPLINE'): its cases, a float64 Cox-de Boor of its own
(neither utils.bspline_basis, which rounds to fp32, nor scipy), the derived bound of the fp32 basis against it, and the float64
definition of every case through pe_curves_cases.definition(..., basis=).  Shapes, event seed, control-point scale and seeds are
those of pe_curves_cases.  Plain module imported by tests."""
import functools

import torch

import pe_curves_cases as PC
import grad_accounting as GA
from oracle import focus_oracle as O

B, M, NB, SP, SHAPE, HQ, WQ = PC.B, PC.M, PC.NB, PC.SP, PC.SHAPE, PC.HQ, PC.WQ

# d x mask x ordering x norm x smoothness x t_ref.  bspline10: L = 8 spans, t_ref = 0.5 lies exactly on a knot.
CASES = {
    'bspline3': dict(curve='BSPLINE', d=3, mask=False, ordered=False, norm='l1', smooth='on_flow_to_tref', t_ref=0.41),
    'bspline4': dict(curve='BSPLINE', d=4, mask=True, ordered=True, norm='l2', smooth='on_flow_to_next', t_ref=0.0),
    'bspline5': dict(curve='BSPLINE', d=5, mask=False, ordered=True, norm='l2', smooth='on_flow_to_tref', t_ref=1.0),
    'bspline10': dict(curve='BSPLINE', d=10, mask=True, ordered=True, norm='l1', smooth='on_flow_to_next', t_ref=0.5),
    'bspline10_atomic': dict(curve='BSPLINE', d=10, mask=True, ordered=False, norm='l2', smooth='on_flow_to_tref', t_ref=0.41),
    'bspline16': dict(curve='BSPLINE', d=16, mask=False, ordered=True, norm='l1', smooth='on_flow_to_tref', t_ref=0.41),
}


def bspline64(times, d):
    """Cox-de Boor in float64 on the clamped knot vector (0, 0, 0, 0, 1/L, ..., (L-1)/L, 1, 1, 1, 1), L = d - 2: the functions
    N_1 .. N_d of the d + 1 (N_0 multiplies P0 = 0) at times clamped to [0, 1]: [n] -> [n, d].  t = 1 belongs to the last span.
    Inner knots are k / L rounded once in float64; 0 / 0 terms are dropped as the recursion's convention has it."""
    L, p = d - 2, 3
    t = times.double().reshape(-1).clamp(0.0, 1.0)
    knots = torch.cat((torch.zeros(p, dtype=torch.float64), torch.arange(L + 1, dtype=torch.float64) / L, torch.ones(p, dtype=torch.float64)))
    n0 = knots.numel() - 1
    N = torch.zeros(t.numel(), n0, dtype=torch.float64)
    for i in range(n0):
        lo, hi = knots[i], knots[i + 1]
        if hi > lo:
            N[:, i] = (((t >= lo) & (t < hi)) | ((t == 1.0) & (hi == 1.0))).double()
    for q in range(1, p + 1):
        Nn = torch.zeros(t.numel(), n0 - q, dtype=torch.float64)
        for i in range(n0 - q):
            a, b = knots[i + q] - knots[i], knots[i + q + 1] - knots[i + 1]
            if a > 0:
                Nn[:, i] += (t - knots[i]) / a * N[:, i]
            if b > 0:
                Nn[:, i] += (knots[i + q + 1] - t) / b * N[:, i + 1]
        N = Nn
    return N[:, 1:d + 1]


# The fp32 lines of the definition against the exact spline, per element:
#   x = fl(tc * L) is off by at most ulp(x) / 2, and a cubic B-spline function's slope in x is at most 3 (at the clamped ends, where
#   N = (1 - x)^3): 3 * ulp(x) / 2.  (Rounding x across a knot changes the span, not the value: the pieces join there.)
#   The recurrence, all terms non-negative inside a span so relative errors do not amplify: per level j a value passes through
#   right (or left) = one subtraction, temp = one division, right * temp = one product and saved + ... = one sum -- 4 roundings of
#   2^-24 relative on its longest path, 3 levels: 12 roundings, (1 + 2^-24)^12 - 1 of a value <= 1.
BSPLINE_ROUNDINGS = 12


def basis_bound(x):
    """Per element: x fp32 tensor (the scaled time tc * L as the definition rounds it) -> float64 bound on |E_fp32 - E_exact|."""
    x = x.float()
    ulp = (torch.nextafter(x, torch.full_like(x, float('inf'))) - x).double()
    return 1.5 * ulp + ((1.0 + 2.0 ** -24) ** BSPLINE_ROUNDINGS - 1.0)


def basis_bound_of_degree(d):
    """The largest value of `basis_bound` over [0, 1] at degree d (x <= L)."""
    return float(basis_bound(torch.tensor(float(d - 2))))


def knot_times(d):
    """0, 1, every knot k / L as fp32 and its two fp32 neighbours (inside [0, 1] or just outside: those are clamped)."""
    L = d - 2
    k = (torch.arange(L + 1, dtype=torch.float64) / L).float()
    up, dn = torch.nextafter(k, torch.full_like(k, 2.0)), torch.nextafter(k, torch.full_like(k, -1.0))
    return torch.cat((torch.tensor([0.0, 1.0]), k, up, dn))


def loss_cfg(name):
    c = CASES[name]
    return PC.loss_cfg(c['norm'], c['smooth'])


def case_inputs(name):
    """(cfg, events [B, M, 6], num_pos, params, up_mask or None) of a case: pe_curves_cases.case_inputs' recipe."""
    c = CASES[name]
    cfg = loss_cfg(name)
    ev, num_pos = O.synth_events(B, M, SHAPE, NB, seed=11, pad_frac=0.1)
    g = torch.Generator().manual_seed(3 + c['d'])
    if c['mask']:
        h, w = SHAPE[0] // 8, SHAPE[1] // 8
        params = torch.randn(B, 2 * c['d'], h, w, generator=g) * 0.5            # (cvx_upsample multiplies by 8)
        mask = torch.randn(B, 576, h, w, generator=g)
    else:
        params = torch.randn(B, 2 * c['d'], HQ, WQ, generator=g) * 4.0
        mask = None
    return cfg, ev, num_pos, params, mask


def define(name, basis=None, dtype=torch.float64):
    """The definition of a case (pe_curves_cases.definition) with E = bspline64, or `basis` (the fp32 mirror), backward done."""
    c = CASES[name]
    cfg, ev, num_pos, params, mask = case_inputs(name)
    d = c['d']
    r = PC.definition(cfg, ev, num_pos, params, mask, c['t_ref'], c['curve'], dtype=dtype, basis=basis or (lambda t: bspline64(t, d)))
    r['loss'].backward()
    return dict(loss=float(r['loss'].detach()), focus=float(r['focus'].detach()), smooth=float(r['smooth'].detach()), iwes=r['iwes'], warped=r['warped'],
                g_rows=r['rows'].grad.reshape(B, HQ * WQ, 2 * d), g_params=r['params'].grad,
                g_mask=r['mask'].grad if r['mask'] is not None else None)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 definition of a case, evaluated once and shared (read only)."""
    return define(name)


def rows_accounting(name, got_rows_grad, label=''):
    """pe_curves_cases.rows_accounting for these cases: d loss / d rows [B, G, 2d] against the definition's, every mismatch explained
    (POINT_TIGHT, the caps of assert_accountable: 1 % mismatching, 25 % explained)."""
    cfg, ev, num_pos, *_ = case_inputs(name)
    ref = reference(name)
    tiles, sign = PC.explained_tiles(cfg, ev, num_pos, ref['warped'], ref['iwes'])
    res = GA.assert_accountable(got_rows_grad.reshape(ref['g_rows'].shape), ref['g_rows'], tiles, tight=GA.POINT_TIGHT, label=label or name)
    if not sign:
        assert res['mismatch'] <= GA.HANDFUL, f'{name}: {res["mismatch"]} elements mismatch with no sign() to explain them'
    return res
