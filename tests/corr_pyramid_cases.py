"""Cases, exact references and the comparator for the correlation pyramid (csrc/corr_pyramid.hip), shared by
tests/test_corr_pyramid_cases_host.py (CPU) and tests/test_gpu_corr_pyramid_cases.py.

Inputs for which every sum is exact.  Feature maps are integers in [-2, 2], cotangents integers in [-1, 1] (fp32, seeded per case).
With L levels every product and every pooled value is a multiple of 4^-(L-1); the case builder asserts, for every output,
A * sqrt(D) * 4^(L-1) < 2^24, where A is the same output computed in float64 on absolute values.  Then every partial sum of every
summation order is an integer multiple of 4^-(L-1) below 2^24 of them: exact in fp32.  So whatever the tiling, the k split and the
order of the partials, the device has to produce

  * where sqrt(D) is a power of two (D = 4, 16, 64, 256): the float64 CPU autograd result through utils.corr_pyramid, bit for bit
    (asserted representable in fp32 first) -- levels and both gradients;
  * elsewhere (D = 8, 132, 160, 512), forward: fp32(exact sum_c fmap1 * P_l) / fp32 sqrt(D), one IEEE fp32 division, P_l pooled in
    float64 from the integers.  Computed here as the float64 quotient rounded to fp32: the same number, since 53 >= 2 * 24 + 2;
  * elsewhere, gradients: each partial is divided and rounded before the gather sums them, so the comparison is the derived bound of
    tests/test_gpu_corr_pyramid.py, gamma(N + 8) * A with N = the concatenated k length (grad_fmap1) and h * w (grad_fmap2).

`plan` restates cp_make_plan, `tiled` restates the kernels' tiling in float64 (tile decode from the linear block index, split ranges,
the concatenated k of grad_fmap1, the reduce and the gather's 4^-l sum over partials, each fp32 rounding the kernels make) and records
which loader paths every product takes: the census the host test asserts.  `tiled` also serves six named mutants."""
import math
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
BM, BK, MAX_SPLIT = 128, 32, 16                         # CP_BM, CP_BK, CP_MAX_SPLIT

# name -> B, D, h, w, level counts, the plan's S1 / S with a cotangent at every level
_SPECS = dict(
    interior=dict(B=1, D=64, h=16, w=16, nl=[2], S1=2, S=2),
    mixed=dict(B=3, D=64, h=12, w=20, nl=[3, 1, 2], S1=2, S=7),
    wide_l1=dict(B=1, D=64, h=24, w=24, nl=[2, 1], S1=4, S=10),
    d256=dict(B=1, D=256, h=8, w=20, nl=[2], S1=1, S=1),
    d160=dict(B=1, D=160, h=16, w=12, nl=[2], S1=1, S=2),
    d132=dict(B=2, D=132, h=9, w=16, nl=[1, 2], S1=1, S=2),
    d512=dict(B=1, D=512, h=4, w=36, nl=[1], S1=1, S=1),
    d8=dict(B=1, D=8, h=16, w=16, nl=[3], S1=2, S=2),
    six_levels=dict(B=1, D=16, h=37, w=45, nl=[6, 2, 4], S1=13, S=16),
    sixteen=dict(B=1, D=4, h=32, w=32, nl=[6] + [1] * 13 + [3, 2], S1=6, S=16),
    offset=dict(B=2, D=16, h=8, w=16, nl=[2, 1], S1=1, S=2),
)
CASES = tuple(_SPECS)
# levels left without a cotangent -> the plan's S then (S1 is sized as if every level had one)
MISSING = {'mixed': ((1,), 6), 'wide_l1': ((0,), 1), 'six_levels': ((0, 3), 12)}
GUARD_CASES = ('mixed', 'six_levels', 'offset')
REPEAT_CASES = ('six_levels', 'sixteen')
MUTANTS = ('drop_last_kblock', 'first_partial_only', 'slot_as_target', 'pitch_as_n', 'no_width_test', 'sample_slot_swapped')


def cdiv(a, b):
    return (a + b - 1) // b


def gamma(n):
    return (n + 8) * U / (1.0 - (n + 8) * U)


def sqrt32(D):
    """sqrt(D) in fp32 as a Python float: cp_plan.sq, and the divisor utils.corr_pyramid promotes to float64."""
    return float(torch.sqrt(torch.tensor(D).float()))


def pow2_scale(D):
    return math.frexp(sqrt32(D))[0] == 0.5


def level_targets(nl):
    return [[t for t, v in enumerate(nl) if v >= l + 1] for l in range(max(nl))]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
_CASE = {}


def case(name):
    """fmap1 [B, D, h, w], fmap2 [T, B, D, h, w], one cotangent per level [n_l, B * h * w, 1, h_l, w_l]: fp32 integers on the CPU."""
    if name not in _CASE:
        s = _SPECS[name]
        B, D, h, w, nl = s['B'], s['D'], s['h'], s['w'], list(s['nl'])
        g = torch.Generator().manual_seed(1 + 7919 * CASES.index(name))
        tix = level_targets(nl)
        f1 = torch.randint(-2, 3, (B, D, h, w), generator=g).float()
        f2 = torch.randint(-2, 3, (len(nl), B, D, h, w), generator=g).float()
        cot = [torch.randint(-1, 2, (len(ts), B * h * w, 1, h >> l, w >> l), generator=g).float() for l, ts in enumerate(tix)]
        _CASE[name] = types.SimpleNamespace(name=name, B=B, D=D, h=h, w=w, hw=h * w, nl=nl, tix=tix, T=len(nl), L=len(tix), f1=f1, f2=f2,
                                            cot=cot, N=[(h >> l) * (w >> l) for l in range(len(tix))], S1=s['S1'], S=s['S'])
    return _CASE[name]


# ---- the plan (cp_make_plan) ----------------------------------------------------------------------------------------------------
def plan(cs, missing=()):
    """S1, S, kblocks, the pitches and the sub-buffer sizes in floats, for cotangents at every level but those in `missing`."""
    B, D, hw = cs.B, cs.D, cs.hw
    n = [len(ts) for ts in cs.tix]
    pitch = [cdiv(v, 4) * 4 for v in cs.N]
    pooled = sum(n[l] * B * D * pitch[l] for l in range(1, cs.L))
    tiles1 = sum(n[l] * max(B, 1) * cdiv(D, BM) * cdiv(cs.N[l], BM) for l in range(cs.L))
    S1 = max(1, min(MAX_SPLIT, cdiv(768, tiles1), cdiv(hw, BK) // 4))
    gp = sum(n[l] * B * D * pitch[l] for l in range(cs.L))
    kblocks = sum(n[l] * cdiv(cs.N[l], BK) for l in range(cs.L) if l not in missing)
    tiles = max(B, 1) * cdiv(D, BM) * cdiv(hw, BM)
    S = max(1, min(MAX_SPLIT, cdiv(768, tiles), kblocks // 4))
    p_off, off = [0] * cs.L, 0
    for l in range(1, cs.L):
        p_off[l], off = off, off + n[l] * B * D * pitch[l]
    return types.SimpleNamespace(S1=S1, S=S, kblocks=kblocks, pitch=pitch, pooled=pooled, gp=gp, part=(S * B * D * hw if S > 1 else 0),
                                 total_bwd=pooled + S1 * gp + (S * B * D * hw if S > 1 else 0), n=n, p_off=p_off)


# ---- the references -------------------------------------------------------------------------------------------------------------
def _autograd64(cs, f1, f2, cot, missing):
    from motionpriorcmax_amd import utils
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    levels, tix = utils.corr_pyramid(a, b, cs.nl)
    assert tix == cs.tix
    keep = [l for l in range(cs.L) if l not in missing]
    g1, g2 = torch.autograd.grad([levels[l] for l in keep], [a, b], [cot[l].double() for l in keep])
    return [lv.detach() for lv in levels], g1, g2


def contract_levels(cs):
    """fp32(exact sum_c fmap1 * P_l / fp32 sqrt(D)) with P_l pooled in float64: the forward the kernel states, as fp32 tensors."""
    B, D, hw = cs.B, cs.D, cs.hw
    a = cs.f1.double().reshape(B, D, hw).transpose(1, 2)
    P, out = cs.f2.double(), []
    for l, ts in enumerate(cs.tix):
        if l:
            pick = [cs.tix[l - 1].index(t) for t in ts]
            P = F.avg_pool2d(P[pick].reshape(-1, 1, cs.h >> (l - 1), cs.w >> (l - 1)), 2, stride=2).reshape(len(ts), B, D, cs.h >> l, cs.w >> l)
        lv = (a @ P.reshape(len(ts), B, D, cs.N[l])) / sqrt32(D)
        out.append(lv.reshape(len(ts), B * hw, 1, cs.h >> l, cs.w >> l).float())
    return out


_EXPECTED = {}
RATIO = {}                                               # case -> {output: the precondition's ratio to 2^24} (printed by the host test)


def expected(name, missing=()):
    """-> levels (fp32, compared bit for bit), g1 / g2 with b1 / b2: fp32 and None where the comparison is bit for bit, float64 and
    the bound tensor elsewhere.  The exactness precondition is asserted here, for every output, on the case with every cotangent."""
    key = (name, tuple(missing))
    if key in _EXPECTED:
        return _EXPECTED[key]
    cs = case(name)
    levels, g1, g2 = _autograd64(cs, cs.f1, cs.f2, cs.cot, missing)
    mags = None
    if not missing or not pow2_scale(cs.D):
        mags = _autograd64(cs, cs.f1.abs(), cs.f2.abs(), [c.abs() for c in cs.cot], missing)
    if not missing:
        scale = sqrt32(cs.D) * 4.0 ** (cs.L - 1)
        RATIO[name] = {k: float(v) * scale / 2.0 ** 24 for k, v in
                       (('levels', max(m.max() for m in mags[0])), ('grad_fmap1', mags[1].max()), ('grad_fmap2', mags[2].max()))}
        assert all(v < 1.0 for v in RATIO[name].values()), (name, RATIO[name])
    e = types.SimpleNamespace(b1=None, b2=None, exact=pow2_scale(cs.D))
    if e.exact:
        for t in levels + [g1, g2]:
            assert torch.equal(t.float().double(), t), f'{name}: the float64 reference is not representable in fp32'
        e.levels, e.g1, e.g2 = [lv.float() for lv in levels], g1.float(), g2.float()
    else:
        e.levels = contract_levels(cs)
        for l, lv in enumerate(e.levels):                 # the contract is itself inside the derived bound of the float64 reference
            assert bool(((lv.double() - levels[l]).abs() <= gamma(cs.D) * mags[0][l]).all())
        kcat = sum(len(ts) * cs.N[l] for l, ts in enumerate(cs.tix) if l not in missing)
        e.g1, e.g2, e.b1, e.b2 = g1, g2, gamma(kcat) * mags[1], gamma(cs.hw) * mags[2]
    _EXPECTED[key] = e
    return e


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def compare(label, output, got, want, bound=None, B=1, book=None):
    """output: 'level_<l>', 'grad_fmap1' or 'grad_fmap2'.  bound None: `got` (fp32) equals `want` (fp32) bit for bit; else
    |got - want| <= bound per element (a non-finite value fails).  Raises an AssertionError that names the first bad element as
    (level, slot, sample, i, j) or (t, b, c, y, x) with both values.  book: a dict that collects per output kind
    [comparisons, elements, elements compared bit for bit, largest error / bound, its label]."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.dtype == torch.float32 and got.numel() == want.numel(), (label, output, got.dtype, tuple(got.shape), tuple(want.shape))
    got = got.reshape(want.shape)
    ratio = 0.0
    if bound is None:
        assert want.dtype == torch.float32
        bad = got.contiguous().view(torch.int32) != (want + 0.0).contiguous().view(torch.int32)       # (+ 0.0: a reference -0 is +0)
    else:
        err = (got.double() - want.double()).abs()
        bad = ~(err <= bound)
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    nbad = int(bad.sum())
    if nbad or not math.isfinite(ratio):
        ratio = float('inf')
    kind = 'levels' if output.startswith('level_') else output
    print(f'{label} {output}: {"bit for bit" if bound is None else f"largest error / bound {ratio:.4f}"}, {got.numel()} elements', flush=True)
    if book is not None:
        ent = book.setdefault(kind, [0, 0, 0, 0.0, ''])
        ent[0] += 1
        ent[1] += got.numel()
        ent[2] += got.numel() if bound is None else 0
        if bound is not None and ratio > ent[3]:
            ent[3:] = [ratio, label]
    if nbad:
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        if kind == 'levels':
            rows = got.shape[1] // B
            where = f'(level {int(output[6:])}, slot {idx[0]}, sample {idx[1] // rows}, i {idx[1] % rows}, j {idx[3] * got.shape[4] + idx[4]})'
        else:
            where = '(t, b, c, y, x) = (' + ', '.join(str(v) for v in (idx if got.dim() == 5 else ('-',) + idx)) + ')'
        tail = '' if bound is None else f', |difference| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e}'
        raise AssertionError(f'{label} {output}: first bad element {where}: got {float(got[idx])!r}, expected {float(want[idx])!r}{tail} '
                             f'({nbad} of {bad.numel()} bad)')
    return ratio


def compare_all(label, name, missing=(), levels=None, g1=None, g2=None, book=None):
    """Whatever is given of the levels (a list) and the two gradients, against expected(name, missing)."""
    cs, e = case(name), expected(name, missing)
    for l, lv in enumerate(levels or ()):
        compare(label, f'level_{l}', lv, e.levels[l], B=cs.B, book=book)
    if g1 is not None:
        compare(label, 'grad_fmap1', g1, e.g1, e.b1, book=book)
    if g2 is not None:
        compare(label, 'grad_fmap2', g2, e.g2, e.b2, book=book)


# ---- the tiling, restated -------------------------------------------------------------------------------------------------------
def _r32(t):
    return t.float().double()


def _loads(paths, product, operand, kc, vec, rem, k0, k1):
    """The branches of cp_load<kc> an operand tile takes over the k blocks of [k0, k1): recorded as (product, operand, path)."""
    for kb in range(k0, k1, BK):
        if vec and rem >= BM and kb + BK <= k1:
            paths.add((product, operand, 'interior'))
            continue
        paths.add((product, operand, 'vec_ragged' if vec else 'scalar'))
        short = (k1 - kb) if kc else rem                  # the extent along the contiguous axis
        if vec and short < (BK if kc else BM) and short % 4:
            paths.add((product, operand, 'tail16'))


def tiled(name, missing=(), mutant=None, aligned=True):
    """The three products block by block as k_corr_pyr_gemm<0 / 1 / 2> decodes them, k_corr_pyr_pool, k_corr_pyr_reduce and
    k_corr_pyr_gather, in float64 with the kernels' fp32 roundings.  -> levels, g1, g2 (fp32; NaN where no block wrote) and `paths`,
    the census.  aligned: whether the operands' bases are 16-byte aligned (decides `vec`, nothing else)."""
    assert mutant is None or mutant in MUTANTS
    cs = case(name)
    P = plan(cs, missing)
    B, D, hw, L, n, N, pitch = cs.B, cs.D, cs.hw, cs.L, P.n, cs.N, P.pitch
    sq = sqrt32(D)
    paths = set()
    f1 = cs.f1.double().reshape(B, D, hw)
    G = [None if l in missing else cs.cot[l].double().reshape(n[l], B * hw, N[l]) for l in range(L)]
    tm_d, vec_hw = cdiv(D, BM), aligned and hw % 4 == 0

    def vrow(l, k, b):                                    # the row offset of (slot, sample) in a level's volume
        return (b * n[l] + k) * hw if mutant == 'sample_slot_swapped' else (k * B + b) * hw

    # k_corr_pyr_pool: P_l [n_l][B][D][pitch_l], the pad 0
    pooled = [cs.f2.double().reshape(cs.T, B, D, hw)]
    for l in range(1, L):
        hp, wp = cs.h >> (l - 1), cs.w >> (l - 1)
        pick = []
        for k, t in enumerate(cs.tix[l]):
            t = k if mutant == 'slot_as_target' else t
            pick.append(cs.tix[l - 1].index(t) if t in cs.tix[l - 1] else n[l - 1] - 1)
        src = pooled[l - 1][pick][..., :N[l - 1]].reshape(n[l], B, D, hp, wp)
        he, we = 2 * (cs.h >> l), 2 * (cs.w >> l)
        q = _r32(_r32(_r32(_r32(src[..., 0:he:2, 0:we:2] + src[..., 0:he:2, 1:we:2]) + src[..., 1:he:2, 0:we:2]) + src[..., 1:he:2, 1:we:2]) * 0.25)
        pooled.append(F.pad(q.reshape(n[l], B, D, N[l]), (0, pitch[l] - N[l])))

    def operand(l, k, b):                                 # cp_pooled: [D, ld] with the valid columns first
        if l and mutant == 'pitch_as_n':
            return pooled[l][k, b].reshape(-1).as_strided((D, N[l]), (N[l], 1))
        return pooled[l][k, b]

    # ---- MODE 0: (level, slot, sample, tile m, tile n), n fastest; m = i, n = j, k = c
    levels = [torch.full((n[l] * B * hw, N[l]), float('nan'), dtype=torch.float64) for l in range(L)]
    tm = cdiv(hw, BM)
    first = [0]
    for l in range(L):
        first.append(first[-1] + n[l] * B * tm * cdiv(N[l], BM))
    for bid in range(first[-1]):
        l = max(v for v in range(L) if first[v] <= bid)
        r, tn = bid - first[l], cdiv(N[l], BM)
        in_, r = r % tn, r // tn
        im, r = r % tm, r // tm
        b, k = r % B, r // B
        m0, n0 = im * BM, in_ * BM
        m1, n1 = min(m0 + BM, hw), min(n0 + BM, N[l])
        _loads(paths, 'fwd', 'A', False, vec_hw, hw - m0, 0, D)
        _loads(paths, 'fwd', 'B', False, l > 0 or vec_hw, N[l] - n0, 0, D)
        paths.update({('fwd', 'm_rem')} if m1 - m0 < BM else ())
        paths.update({('fwd', 'n_rem')} if n1 - n0 < BM else ())
        paths.update({('fwd', 'k_rem')} if D % BK else ())
        paths.update({('fwd', 'n_tiles_above_0')} if l > 0 and tn > 1 else ())
        acc = f1[b][:, m0:m1].T @ operand(l, k, b)[:, n0:n1]
        levels[l][vrow(l, k, b) + m0:vrow(l, k, b) + m1, n0:n1] = _r32(acc / sq)

    # ---- MODE 1: (level with a cotangent, split, slot, sample, tile m, tile n); m = c, n = j, k = i
    gp = [torch.full((P.S1, n[l], B, D, pitch[l]), float('nan'), dtype=torch.float64) for l in range(L)]
    first = [0]
    for l in range(L):
        first.append(first[-1] + (0 if l in missing else P.S1 * n[l] * B * tm_d * cdiv(N[l], BM)))
    nkb = cdiv(hw, BK)
    for bid in range(first[-1]):
        l = max(v for v in range(L) if first[v] <= bid and first[v + 1] > first[v])
        r, tn = bid - first[l], cdiv(N[l], BM)
        per = n[l] * B * tm_d * tn
        s, r = r // per, r % per
        in_, r = r % tn, r // tn
        im, r = r % tm_d, r // tm_d
        b, k = r % B, r // B
        m0, n0 = im * BM, in_ * BM
        m1, n1 = min(m0 + BM, D), min(n0 + BM, N[l])
        kb0, kb1 = s * nkb // P.S1, (s + 1) * nkb // P.S1
        if mutant == 'drop_last_kblock' and kb1 - kb0 > 1:
            kb1 -= 1
        k0, k1 = kb0 * BK, min(kb1 * BK, hw)
        _loads(paths, 'gP', 'A', True, vec_hw, D - m0, k0, k1)
        _loads(paths, 'gP', 'B', False, aligned and N[l] % 4 == 0, N[l] - n0, k0, k1)
        paths.update({('gP', 'm_rem')} if m1 - m0 < BM else ())
        paths.update({('gP', 'm_rem_late')} if m1 - m0 < BM and im > 0 else ())
        paths.update({('gP', 'n_rem')} if n1 - n0 < BM else ())
        paths.update({('gP', 'k_rem')} if (k1 - k0) % BK else ())
        paths.update({('gP', 'n_tiles_above_0')} if l > 0 and tn > 1 else ())
        paths.update({('gP', 'split')} if P.S1 > 1 else ())
        paths.update({('gP', 'uneven_ranges')} if nkb % P.S1 else ())
        paths.update({('gP', 'range_ends_in_ragged_block')} if P.S1 > 1 and kb1 * BK > hw else ())
        g = G[l].reshape(-1, N[l])[vrow(l, k, b) + k0:vrow(l, k, b) + k1, n0:n1]
        acc = f1[b][m0:m1, k0:k1] @ g
        gp[l][s, k, b, m0:m1, n0:n1] = _r32(acc / sq)

    # ---- MODE 2: (split, sample, tile m, tile n); m = c, n = i, k = the concatenation over (level, slot, j) in k blocks
    tn = cdiv(hw, BM)
    part = torch.full((P.S, B, D, hw), float('nan'), dtype=torch.float64)
    segs = [(l, k) for l in range(L) if l not in missing for k in range(n[l])]
    for bid in range(P.S * B * tm_d * tn):
        in_, r = bid % tn, bid // tn
        im, r = r % tm_d, r // tm_d
        b, s = r % B, r // B
        m0, n0 = im * BM, in_ * BM
        m1, n1 = min(m0 + BM, D), min(n0 + BM, hw)
        kb0, kb1 = s * P.kblocks // P.S, (s + 1) * P.kblocks // P.S
        if mutant == 'drop_last_kblock' and kb1 - kb0 > 1:
            kb1 -= 1
        acc = torch.zeros(m1 - m0, n1 - n0, dtype=torch.float64)
        at = 0
        for l, k in segs:
            nb = cdiv(N[l], BK)
            lo, hi = max(kb0, at) - at, min(kb1, at + nb) - at
            at += nb
            if lo >= hi:
                continue
            k0, k1 = lo * BK, min(hi * BK, N[l])
            _loads(paths, 'g1', 'A', True, l > 0 or vec_hw, D - m0, k0, k1)
            _loads(paths, 'g1', 'B', True, aligned and N[l] % 4 == 0, hw - n0, k0, k1)
            paths.update({('g1', 'k_rem')} if (k1 - k0) % BK else ())
            paths.update({('g1', 'range_ends_in_ragged_block')} if s + 1 < P.S and hi == nb and kb1 == at and N[l] % BK else ())
            paths.update({('g1', 'level_1x1')} if N[l] == 1 else ())
            g = G[l].reshape(-1, N[l])[vrow(l, k, b) + n0:vrow(l, k, b) + n1, k0:k1]
            acc = acc + operand(l, k, b)[m0:m1, k0:k1] @ g.T
        paths.update({('g1', 'm_rem')} if m1 - m0 < BM else ())
        paths.update({('g1', 'm_rem_late')} if m1 - m0 < BM and im > 0 else ())
        paths.update({('g1', 'n_rem')} if n1 - n0 < BM else ())
        paths.update({('g1', 'split')} if P.S > 1 else ())
        paths.update({('g1', 'split_cap')} if P.S == MAX_SPLIT else ())
        paths.update({('g1', 'uneven_ranges')} if P.kblocks % P.S else ())
        paths.update({('g1', 'missing_cotangent_split')} if P.S > 1 and missing else ())
        part[s, b, m0:m1, n0:n1] = _r32(acc / sq) if P.S == 1 else _r32(acc)
    v = part[0]                                           # k_corr_pyr_reduce: the partials in index order, then the division
    for s in range(1, P.S):
        v = _r32(v + part[s])
    g1 = (v if P.S == 1 else _r32(v / sq)).reshape(B, D, cs.h, cs.w)

    # ---- k_corr_pyr_gather: levels ascending, the partials of a level in index order, weight 4^-l
    g2 = torch.zeros(cs.T, B, D, cs.h, cs.w, dtype=torch.float64)
    ys, xs = torch.arange(cs.h), torch.arange(cs.w)
    for l in range(L):
        if l in missing:
            continue
        hl, wl = cs.h >> l, cs.w >> l
        yl, xl = ys >> l, xs >> l
        ok = (yl < hl)[:, None] & ((xl < wl)[None] if mutant != 'no_width_test' else torch.ones(1, cs.w, dtype=torch.bool))
        for k, t in enumerate(cs.tix[l]):
            for s in range(1 if mutant == 'first_partial_only' else P.S1):
                src = gp[l][s, k][..., :N[l]].reshape(B, D, hl, wl)[:, :, yl.clamp(max=hl - 1)][:, :, :, xl.clamp(max=wl - 1)]
                g2[t] = torch.where(ok, _r32(g2[t] + 0.25 ** l * src), g2[t])
    paths.add(('gather', 'V4' if aligned and cs.w % 4 == 0 else 'V1'))
    paths.update({('gather', 'V4_partials')} if aligned and cs.w % 4 == 0 and P.S1 > 1 else ())
    paths.update({('gather', 'level_1x1')} if any(N[l] == 1 and l not in missing for l in range(L)) else ())
    out_levels = [lv.float().reshape(n[l], B * hw, 1, cs.h >> l, cs.w >> l) for l, lv in enumerate(levels)]
    return types.SimpleNamespace(levels=out_levels, g1=g1.float(), g2=g2.float(), paths=paths, plan=P)
