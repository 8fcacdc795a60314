"""Cases and exact references for the correlation pyramid over several references (the events-plus-frames merge: utils.corr_pyramid in
list form, ops.CorrPyramidMultiFn, csrc/corr_pyramid.hip), shared by tests/test_corr_pyramid_multi_host.py (CPU) and
tests/test_gpu_corr_pyramid_multi.py.  In the manner of tests/corr_pyramid_cases.py (PK), whose comparator, gamma and plan serve here.

Inputs for which every sum is exact: feature maps integers in [-2, 2] (a spec may narrow the range, never the rule), cotangents
integers in [-1, 1], fp32, seeded per case.  With L levels every product and every pooled value is a multiple of 4^-(L-1); the builder
asserts, for every output, A * sqrt(D) * 4^(L-1) < 2^24 with A the same output computed in float64 on absolute values.  Then, whatever
the tiling, the k split and the order of the partials,

  * where sqrt(D) is a power of two: levels and all 2R gradients are the float64 autograd result through the list-form utils.corr_pyramid,
    bit for bit (asserted representable in fp32 first);
  * elsewhere (D = 132): the levels are fp32(exact sum / fp32 sqrt(D)), one correctly rounded division (PK.contract_levels per
    reference, merged by slot range); the gradients take the derived bound of PK per reference, gamma(N + 8) * A with N the
    concatenated k length of THAT reference's (level, slot, j) for grad_fmap1 and h * w for grad_fmap2 -- the problem is block-diagonal,
    no sum runs across references.

The flat target list is the concatenation of the references' targets; level l holds the flat targets with more than l levels,
ascending, so the slots of a reference are contiguous in every level: `slots(cs, r, l)`."""
import types

import torch

import corr_pyramid_cases as PK

# name -> B, D, h, w, the level counts per reference, the value range of the feature maps
_SPECS = dict(
    base_model=dict(B=1, D=64, h=16, w=24, nls=[[1, 2, 3, 4], [4]]),
    stops_at_0=dict(B=3, D=64, h=12, w=20, nls=[[1, 1], [3]]),
    three_ragged=dict(B=1, D=132, h=9, w=13, nls=[[2], [1, 3], [1]]),
    sixteen=dict(B=1, D=4, h=32, w=32, nls=[[6, 1, 1, 1], [1, 1, 1, 1, 1, 1], [3, 2, 1], [1, 1, 4]]),
    offset=dict(B=1, D=64, h=8, w=16, nls=[[1, 2, 3, 4], [4]]),
)
CASES = tuple(_SPECS)
# levels left without a cotangent
MISSING = {'base_model': (1, 3), 'stops_at_0': (0,), 'three_ragged': (1,), 'sixteen': (0, 4)}
# which of the 2R gradients are asked for: (fmap1 per reference, fmap2 per reference)
PARTIAL = {
    'base_model': [((False, True), (False, True)), ((True, False), (False, False)), ((False, False), (True, False))],
    'stops_at_0': [((False, True), (False, True)), ((True, False), (True, False)), ((False, True), (True, False))],
    'three_ragged': [((False, True, False), (True, False, True))],
}

_CASE = {}


def case(name):
    """f1[r] [B, D, h, w], f2[r] [n_r, B, D, h, w], one cotangent per merged level [n_l, B * h * w, 1, h_l, w_l]: fp32 integers (CPU)."""
    if name not in _CASE:
        s = _SPECS[name]
        B, D, h, w, nls = s['B'], s['D'], s['h'], s['w'], [list(v) for v in s['nls']]
        lo, hi = s.get('range', (-2, 2))
        g = torch.Generator().manual_seed(23 + 7919 * CASES.index(name))
        nl = [v for ref in nls for v in ref]
        tix = PK.level_targets(nl)
        first = [0]
        for ref in nls:
            first.append(first[-1] + len(ref))
        f1 = [torch.randint(lo, hi + 1, (B, D, h, w), generator=g).float() for _ in nls]
        f2 = [torch.randint(lo, hi + 1, (len(ref), B, D, h, w), generator=g).float() for ref in nls]
        cot = [torch.randint(-1, 2, (len(ts), B * h * w, 1, h >> l, w >> l), generator=g).float() for l, ts in enumerate(tix)]
        _CASE[name] = types.SimpleNamespace(name=name, B=B, D=D, h=h, w=w, hw=h * w, nls=nls, nl=nl, tix=tix, R=len(nls), T=len(nl),
                                            L=len(tix), first=first, f1=f1, f2=f2, cot=cot, N=[(h >> l) * (w >> l) for l in range(len(tix))])
    return _CASE[name]


def slots(cs, r, l):
    """(first slot, slot count) of reference r in level l."""
    own = [k for k, t in enumerate(cs.tix[l]) if cs.first[r] <= t < cs.first[r + 1]]
    assert own == list(range(own[0], own[0] + len(own))) if own else True
    return (own[0], len(own)) if own else (0, 0)


def reference_case(cs, r, missing=()):
    """Reference r alone as a case of PK (f1, f2, nl, tix, its slice of every cotangent): what the tensor form takes for it."""
    nl = cs.nls[r]
    tix = PK.level_targets(nl)
    cot = [cs.cot[l][slots(cs, r, l)[0]:sum(slots(cs, r, l))] for l in range(len(tix))]
    return types.SimpleNamespace(name=f'{cs.name}[{r}]', B=cs.B, D=cs.D, h=cs.h, w=cs.w, hw=cs.hw, nl=nl, tix=tix, T=len(nl), L=len(tix),
                                 f1=cs.f1[r], f2=cs.f2[r], cot=cot, N=cs.N[:len(tix)])


def merge(cs, per_reference):
    """Levels of the references taken alone (a list per reference) -> the merged levels: slot ranges in reference order."""
    return [torch.cat([lv[l] for lv in per_reference if l < len(lv)], dim=0) for l in range(cs.L)]


def split_plan(cs, r, missing=()):
    """PK.plan of reference r alone: the S1 / S / kblocks the multi-reference call keeps for it."""
    rc = reference_case(cs, r)
    return PK.plan(rc, tuple(l for l in missing if l < rc.L))


def _autograd64(cs, f1, f2, cot, missing):
    from motionpriorcmax_amd import utils
    a = [t.double().requires_grad_(True) for t in f1]
    b = [t.double().requires_grad_(True) for t in f2]
    levels, tix = utils.corr_pyramid(a, b, cs.nls)
    assert tix == cs.tix
    keep = [l for l in range(cs.L) if l not in missing]
    grads = torch.autograd.grad([levels[l] for l in keep], a + b, [cot[l].double() for l in keep], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, a + b)]          # (no level reaches the reference: zero)
    return [lv.detach() for lv in levels], grads[:cs.R], grads[cs.R:]


_EXPECTED = {}
RATIO = {}                                               # case -> {output: the precondition's ratio to 2^24}


def expected(name, missing=()):
    """-> levels (fp32, bit for bit), g1[r] / g2[r] with b1[r] / b2[r]: fp32 and None where the comparison is bit for bit, float64
    and the bound tensor elsewhere (there also levels64 / levels_abs: the float64 levels and those of the absolute values).  The
    exactness precondition is asserted here, for every output, on the case with every cotangent."""
    key = (name, tuple(missing))
    if key in _EXPECTED:
        return _EXPECTED[key]
    cs = case(name)
    levels, g1, g2 = _autograd64(cs, cs.f1, cs.f2, cs.cot, missing)
    mags = None
    if not missing or not PK.pow2_scale(cs.D):
        mags = _autograd64(cs, [t.abs() for t in cs.f1], [t.abs() for t in cs.f2], [c.abs() for c in cs.cot], missing)
    if not missing:
        scale = PK.sqrt32(cs.D) * 4.0 ** (cs.L - 1)
        RATIO[name] = {k: float(v) * scale / 2.0 ** 24 for k, v in
                       (('levels', max(m.max() for m in mags[0])), ('grad_fmap1', max(m.max() for m in mags[1])),
                        ('grad_fmap2', max(m.max() for m in mags[2])))}
        assert all(v < 1.0 for v in RATIO[name].values()), (name, RATIO[name])
    e = types.SimpleNamespace(b1=[None] * cs.R, b2=[None] * cs.R, exact=PK.pow2_scale(cs.D))
    if e.exact:
        for t in levels + g1 + g2:
            assert torch.equal(t.float().double(), t), f'{name}: the float64 reference is not representable in fp32'
        e.levels, e.g1, e.g2 = [lv.float() for lv in levels], [g.float() for g in g1], [g.float() for g in g2]
    else:
        e.levels = merge(cs, [PK.contract_levels(reference_case(cs, r)) for r in range(cs.R)])
        for l, lv in enumerate(e.levels):                 # the contract is itself inside the derived bound of the float64 reference
            assert bool(((lv.double() - levels[l]).abs() <= PK.gamma(cs.D) * mags[0][l]).all())
        e.g1, e.g2, e.levels64, e.levels_abs = g1, g2, levels, mags[0]
        for r in range(cs.R):
            kcat = sum(slots(cs, r, l)[1] * cs.N[l] for l in range(len(PK.level_targets(cs.nls[r]))) if l not in missing)
            e.b1[r], e.b2[r] = PK.gamma(kcat) * mags[1][r], PK.gamma(cs.hw) * mags[2][r]
    _EXPECTED[key] = e
    return e


def compare_all(label, name, missing=(), levels=None, g1=None, g2=None, book=None):
    """Whatever is given of the levels (a list) and the gradients (lists over the references, None entries skipped), against
    expected(name, missing), with PK.compare."""
    cs, e = case(name), expected(name, missing)
    for l, lv in enumerate(levels or ()):
        PK.compare(label, f'level_{l}', lv, e.levels[l], B=cs.B, book=book)
    for r in range(cs.R):
        if g1 is not None and g1[r] is not None:
            PK.compare(f'{label} reference {r}', 'grad_fmap1', g1[r], e.g1[r], e.b1[r], book=book)
        if g2 is not None and g2[r] is not None:
            PK.compare(f'{label} reference {r}', 'grad_fmap2', g2[r], e.g2[r], e.b2[r], book=book)
