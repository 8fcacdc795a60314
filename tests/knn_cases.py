"""Named cases of the KNN flow LUT (csrc/knn.hip, knn_strip.hip, knn_device.h), their reference, and the rules by which the
saved state, every output element and every neighbour list is compared with it.  A helper module (no fixtures):
tests/test_knn_cases_host.py checks the cases, the reference and the comparator on the CPU (a float32 stand-in of the whole
operation passes, eleven mutants of it fail, each by the name of the assertion meant to catch it),
tests/test_gpu_knn_cases.py runs the cases on the device.

Inputs.  The search reads only the mid-time rows of the trajectories, so a case takes those from a geometry that steers the
route (lattice, flow family, piles, bands, ...) and its reference-time rows are mid row 0 + e, e uniform in [-8, 8]^2 per point:
the flow of a point has nothing to do with where it lies, and exchanging one neighbour for another moves the LUT by about
|e - e'| / K.  separation() measures that for every query: the K-th neighbour replaced by the (K + 1)-th.

Selection.  Ranked in float32 with the operand order of focus.py:132-135 (knn_wide_cases.distances), ordered by (distance,
index) (knn_wide_cases.ordered_knn): the kernels' own arithmetic (pair_dist, knn_device.h:169-173, -ffp-contract=off), so the
neighbour sets are the same on both sides bit for bit, ties included, and no query is excused.

Values.  float64 over those sets: 'mean', 'iwd' (1 / (d + 1e-9), d in float64 from the positions; K == 1 is a plain gather,
focus.py:145-147), flow_next (always a mean), and the exact adjoint with respect to every row ('iwd' weights are constants).

Allowances.  gamma(k) = k u / (1 - k u), u = 2^-24, times the same chain on absolute values.  The sums run in bucket order,
lane order or a shuffle tree, so every sum of m terms takes the order-free bound of m - 1 additions (an addition of an exact
zero -- a slot that is no neighbour, an empty lane -- rounds nothing).  k per kernel, longest path, with the source lines:

  flow of a point          1   traj(t_ref) - traj(t_mid), one subtraction: knn_strip.hip:455-456, 1199, 1202; knn_device.h:220, 225
  D  distance              4   'l2': q - p (1), its square (2 more: the error of q - p twice, the product once), the sum (1);
                           2   'l1': q - p (1), the sum (1).  The cell centre cy * sp + off is exact.   pair_dist, knn_device.h:169-173
  W  'iwd' weight      D + 4   d + 1e-9f (1, and 1 for the constant 1e-9f against 1e-9), the reciprocal: v_rcp_f32 at 1 ulp =
                               2 u on the strip path and in the tile gather (ks_iwd_weight, knn_strip.hip:93; knn.hip:783, 1102,
                               1121), one IEEE division (1) elsewhere (knn_device.h:390, 424, 448, 488, 545; knn_strip.hip:1200;
                               knn.hip:716)
  strip pass 2, 'mean'     K + 1   flow 1, K - 1 additions (fmaf with a flag of 128.0 or 0.0: knn_strip.hip:641; the factor 128
                               is a power of two), the K-th level light (:691) or heavy (:740 lane sums, :747 shuffle tree, :758
                               fmaf(128, c, s)) -- still K - 1 additions in all --, then sum * 2^-(7 + log2 K), exact (:775), or
                               (sum * 2^-7) / K: 1 (:776).  flow_next the same (:642, 692, 741, 749, 759, 780-781)
  strip pass 2, 'iwd'      numerator W + 1 (flow) + 1 (the product: fused at :640 and :690, separate at :740) + K - 1;
                           normaliser N = W + K - 1 (:640, 690, 740, 748, 757); the quotient 1 (:769): 2 W + 2 K + 1.
                           The saved normaliser is sw * 2^-7, exact (:769): N
  one-wavefront fallback   fallback_one_query: 'mean' K + 1: flow 1 (:1199), lane sums and shuffle tree K - 1 (:1201, 1206-1209),
                           / K 1 (:1218); 'iwd' as the strip's with the separate product (:1200) and IEEE divisions (:1217):
                           <= 2 W + 2 K + 1
  k_knn_query              knn_one_query, knn_device.h: 'mean' K + 1 (:220, 391, 425, 449, 489, 548, 525, 558); 'iwd'
                           <= 2 W + 2 K + 1 (:390, 424, 448, 488, 545-546, 524, 557); T flows: the same per reference time
  tile gather              k_knn_bwd_tile, per point and bin: 'mean' the member gradients K-free: M - 1 additions over its M
                           members (knn.hip:785, 1103, 1122), 1 / K rounded (1, :1040-1041) and the product (1, :1132, 1134): C = 2;
                           'iwd': the staged gradient is dL/dLUT / normaliser (1, :1012, and the normaliser's own N), the weight W,
                           the product fused (:783-784, 1102) -- or rcp((d + 1e-9) * normaliser), one product more (:1121):
                           C = W + N + 2.  The flow_next sums are means in both schemes (:786, 1104, 1123, 1135)
  far backward             k_knn_bwd_far: integer sums of round(g * 2^(40 - ex)), 2^ex the power of two above the largest
                           |gradient| of the list (knn.hip:1244-1246): at most |g|max * 2^-40 per add (:1326-1330), then the
                           conversion (1, :1347), 1 / K and its product (2) and the addition to the gather's value (:1351,
                           1355: one of the M - 1): C = 3; 'iwd' (1 / (d + 1e-9)) / normaliser (W + N + 1), times g (1, :1325-1327)
                           and the conversion (1): C = W + N + 3
  k_knn_bwd_points         num_tref > 1: w = 1 / K (1, knn.hip:683), ay += w * g (product 1, :716-717), flow_next the same (:718): C = 2;
                           'iwd': w = (1 / (d + 1e-9)) / normaliser (W + N + 1, :716) and the product (1): C = W + N + 2
  combines                 k_knn_bwd_combine (knn.hip:1385, 1394, 1397), _bins (:1422-1423, 1430), _direct (:1448): additions of the
                           per-bin values only; with all members of an element counted in M they are among its M - 1 additions

So per element: flow_lut 'mean' and flow_next gamma(K + 1) mean|flow|; flow_lut 'iwd' gamma(2 W + 2 K + 1) sum(w |flow|) / sum(w);
normaliser gamma(W + K - 1) sum(w); grad_traj gamma(C + M) S + M |g|max 2^-40 with M the addends that meet in the element (over
bins, reference times and the flow_next terms), S the sum of their absolute values and C = 3 ('mean') or W + N + 3 ('iwd').  An
element with M = 0 -- a point that is nobody's neighbour -- has allowance zero and must be exactly zero.  These are counted
bounds, not measurements."""
import functools
import math
from dataclasses import dataclass

import torch

from knn_wide_cases import distances, ordered_knn

U = 2.0 ** -24
KNN_TIE_FLAG, KNN_FAR_FLAG, KNN_IDX_MASK = 0x40000000, 0x20000000, 0x1fffffff      # knn_device.h:11-15
KNN_NCLS, KNN_RCAP, KNN_RFAR, KNN_FAR_RINGS = 5, 6, 20, 2                          # knn_device.h:22, 42; tuning.h:154, 157
KNN_MARGIN = KNN_RCAP + 1                                                          # knn_device.h:44
KS_MAXCH, KS_MAXCH_L1, KS_MAXCH_FAR, KS_LMAX, KS_FORWARD_MAX = 24, 32, 48, 4, 1024  # knn_strip.hip:57, 62, 68; tuning.h:113, 120
MPC_KNN_LDS_SORT_CELLS = 150 * 1024 // 4                                           # common.h:11
SEPARATION = 20.0
FAR_QUANTUM = 2.0 ** -40


def gamma(k):
    return k * U / (1.0 - k * U)


def n_dist(norm):
    return 4 if norm == 'l2' else 2


def n_weight(norm):
    return n_dist(norm) + 4


def n_mean(K):
    return K + 1


def n_norm(K, norm):
    return n_weight(norm) + K - 1


def n_iwd(K, norm):
    return 2 * n_weight(norm) + 2 * K + 1


def n_grad(K, norm, iwd):
    return n_weight(norm) + n_norm(K, norm) + 3 if iwd else 3


# ---- the case --------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    H: int
    W: int
    sp: int
    K: int
    norm: str
    scheme: str
    want_next: bool
    T: int
    traj: torch.Tensor                      # [B, T + nb, n, 2] float32 (y, x), reference rows first
    expect: tuple = ()                      # (counter, op, value) the device run must show, see routes() of the GPU file
    note: str = ''

    @property
    def B(self):
        return self.traj.shape[0]

    @property
    def nb(self):
        return self.traj.shape[1] - self.T

    @property
    def n(self):
        return self.traj.shape[2]

    @property
    def hq(self):
        return (self.H + self.sp - 1) // self.sp

    @property
    def wq(self):
        return (self.W + self.sp - 1) // self.sp

    @property
    def iwd(self):
        return self.scheme == 'iwd' and self.K > 1              # knn_device.h:108, focus.py:145-147

    @property
    def has_next(self):
        return self.want_next and self.nb > 1

    def queries(self):
        """Cell centres (y, x) [hq * wq, 2] of the case's own grid, focus.py:116-126."""
        off = self.sp / 2 - 0.5
        gy, gx = torch.meshgrid(torch.arange(0, self.H, self.sp, dtype=torch.float32) + off,
                                torch.arange(0, self.W, self.sp, dtype=torch.float32) + off, indexing='ij')
        return torch.stack((gy, gx), -1).reshape(-1, 2)

    def cotangents(self):
        """dL/dflow_lut [B, nb, hq, wq, T, 2] and dL/dflow_next [B, nb - 1, hq, wq, 1, 2] (or None), seeded."""
        g = torch.Generator().manual_seed(977)
        g_lut = torch.randn(self.B, self.nb, self.hq, self.wq, self.T, 2, generator=g)
        g_next = torch.randn(self.B, self.nb - 1, self.hq, self.wq, 1, 2, generator=g) if self.has_next else None
        return g_lut, g_next


# ---- the library's plans, restated ---------------------------------------------------------------------------------------------
def r_init(c):
    """mpc_knn_r_init, knn.hip:1460-1466."""
    dens = c.n / (c.hq * c.wq)
    ball = 2.0 if c.norm == 'l1' else 3.14159265
    return max(int(math.ceil(math.sqrt(c.K / ball / (dens if dens > 0 else 1.0)) - 0.5)), 1)


def strip_usable(c):
    """mpc_knn_strip_usable and strip_geometry, knn_strip.hip:1335-1362: does the forward of this case run the strip kernel (and the backward the far list)?"""
    r = r_init(c)
    maxch = KS_MAXCH_L1 if c.norm == 'l1' else KS_MAXCH
    if c.T != 1 or c.n >= 65536 or c.K < 1 or c.K > 4 * maxch or c.hq < 2 * r + 2 or c.wq < 2 * r + 2 or r > KNN_RCAP:
        return False
    TH = 128
    row_pts = c.n / (c.hq * c.wq) * (2 + 2 * r)
    if (2 * r + 1) * (row_pts + 0.5) * 1.3 > 4 * maxch:
        return False
    cap = (int(1.15 * (min(TH, c.hq) + 2 * r) * (row_pts + 0.5)) + 32 + 15) // 16 * 16
    NR, tail = TH + 2 * KNN_RFAR, 4 * KS_MAXCH_FAR + 8
    lds_far = ((NR * 8 + (NR + 1) * 4 + 15) & ~15) + (cap + tail) * 8 * (3 if c.want_next else 2) + cap * 2 + 16
    return lds_far <= 64 * 1024


def sort_plan(c):
    """knn_sort_plan, knn.hip:1486-1498 -> (S workgroups per (sample, bin), global-memory sort?)."""
    hb, wb = c.hq + 2 * KNN_MARGIN, c.wq + 2 * KNN_MARGIN
    S = max(min(256 // (c.B * c.nb), 8, hb), 1)
    tail = (c.n + 1) // 2 * 2 * 2 + (c.n + 31) // 32 * 4
    if S == 1:
        tail = max(tail, (hb + 7) // 8 * (wb + 1) * 4)
    lds = (hb + S - 1) // S * wb * 4 + tail
    return S, hb * wb > MPC_KNN_LDS_SORT_CELLS or lds > 145 * 1024


def far_limit(c):
    """knn_is_far_dk, knn_device.h:665-668: a K-th distance beyond it is the far backward's (where the forward is the strip kernel)."""
    lim = torch.tensor((r_init(c) + KNN_FAR_RINGS) + 0.5, dtype=torch.float32) * torch.tensor(float(c.sp), dtype=torch.float32)
    return lim if c.norm == 'l1' else lim * lim


def query_classes(c):
    """knn_query_classes, knn_device.h:601-604 with bd = r_init + 1 (knn_band_depth, :595) -> [hq * wq, 5] bool, and the 16 x 16 tile of every query (:152-153, 610)."""
    bd = r_init(c) + 1
    cy, cx = torch.meshgrid(torch.arange(c.hq), torch.arange(c.wq), indexing='ij')
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    b = torch.stack((cy < bd, cy >= c.hq - bd, cx < bd, cx >= c.wq - bd), 1)
    cls = torch.cat((~b.any(1, keepdim=True), b), 1)
    return cls, (cy // 16) * ((c.wq + 15) // 16) + cx // 16


def num_tiles(c):
    return ((c.hq + 15) // 16) * ((c.wq + 15) // 16)


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _select(c):
    """-> idx [B, nb, Q, K] int64 ordered by (float32 distance, index), the (K + 1)-th neighbour [B, nb, Q] (-1 where n == K) and
    the float32 distances of the K (+ 1) [B, nb, Q, K (+ 1)]; queries in chunks."""
    q = c.queries()
    m = min(c.K + 1, c.n)
    step = max(1, (1 << 25) // max(c.n, 1))
    idx, dist = [], []
    for b in range(c.B):
        for t in range(c.nb):
            pts = c.traj[b, c.T + t]
            parts = [ordered_knn(distances(q[s:s + step], pts, c.norm), m) for s in range(0, q.shape[0], step)]
            idx.append(torch.cat([p[0] for p in parts]))
            dist.append(torch.cat([p[1] for p in parts]))
    Q = q.shape[0]
    return torch.stack(idx).reshape(c.B, c.nb, Q, m), torch.stack(dist).reshape(c.B, c.nb, Q, m)


def _weights(c, b, t, idx):
    """'iwd' weights 1 / (d + 1e-9) in float64 from the positions, [Q, K] (not normalised)."""
    q = c.queries().double()
    diff = q[:, None, :] - c.traj[b, c.T + t].double()[idx]
    d = (diff ** 2).sum(-1) if c.norm == 'l2' else diff.abs().sum(-1)
    return 1.0 / (d + 1e-9)


def _values(c, idx):
    """float64 LUT, flow_next, normaliser and their allowances over the neighbour sets idx [B, nb, Q, K]."""
    tj = c.traj.double()
    K = c.K
    lut, lut_a, nxt, nxt_a, nrm, nrm_a = [], [], [], [], [], []
    for b in range(c.B):
        for t in range(c.nb):
            i = idx[b, t]
            f = (tj[b, :c.T].permute(1, 0, 2) - tj[b, c.T + t][:, None, :])[i]                 # [Q, K, T, 2]
            if c.iwd:
                w = _weights(c, b, t, i)
                ws = w.sum(1)
                lut.append((w[..., None, None] * f).sum(1) / ws[:, None, None])
                lut_a.append(gamma(n_iwd(K, c.norm)) * (w[..., None, None] * f.abs()).sum(1) / ws[:, None, None])
                nrm.append(ws)
                nrm_a.append(gamma(n_norm(K, c.norm)) * ws)
            else:
                lut.append(f.mean(1))
                lut_a.append(gamma(n_mean(K)) * f.abs().mean(1))
                nrm.append(torch.zeros(i.shape[0], dtype=torch.float64))
                nrm_a.append(torch.zeros(i.shape[0], dtype=torch.float64))
            if c.has_next and t < c.nb - 1:
                fn = (tj[b, c.T + t + 1] - tj[b, c.T + t])[i]                                    # [Q, K, 2]
                nxt.append(fn.mean(1))
                nxt_a.append(gamma(n_mean(K)) * fn.abs().mean(1))
    shp = (c.B, c.nb, c.hq, c.wq, c.T, 2)
    out = dict(lut=torch.stack(lut).reshape(shp), lut_allow=torch.stack(lut_a).reshape(shp),
               norm=torch.stack(nrm).reshape(c.B, c.nb, -1), norm_allow=torch.stack(nrm_a).reshape(c.B, c.nb, -1), nxt=None, nxt_allow=None)
    if c.has_next:
        shp = (c.B, c.nb - 1, c.hq, c.wq, 1, 2)
        out['nxt'], out['nxt_allow'] = torch.stack(nxt).reshape(shp), torch.stack(nxt_a).reshape(shp)
    return out


def _adjoint(c, idx, g_lut, g_next, dtype=torch.float64, member=None):
    """The exact adjoint over the neighbour sets -> (grad [B, T + nb, n, 2], sum of |addends|, number of addends [B, T + nb, n]).
    member [B, nb, Q, K] bool masks addends out (the stand-in's mutants); dtype float32 is the stand-in."""
    T, K = c.T, c.K
    grad = torch.zeros(c.B, T + c.nb, c.n, 2, dtype=dtype)
    S = torch.zeros_like(grad)
    M = torch.zeros(c.B, T + c.nb, c.n, dtype=torch.int64)
    Q = idx.shape[2]
    invK = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(K), dtype=dtype)
    for b in range(c.B):
        for t in range(c.nb):
            i = idx[b, t]
            flat = i.reshape(-1)
            if c.iwd:
                w = _weights(c, b, t, i)
                w = (w / w.sum(1, keepdim=True)).to(dtype)
            else:
                w = invK.expand(Q, K)
            on = torch.ones(Q, K, dtype=torch.bool) if member is None else member[b, t]
            w = w * on.to(dtype)
            cnt = torch.zeros(c.n, dtype=torch.int64).index_add_(0, flat, on.reshape(-1).long())
            gl = g_lut[b, t].reshape(Q, T, 2).to(dtype)
            for tr in range(T):
                con = (w[:, :, None] * gl[:, None, tr, :]).reshape(-1, 2)
                grad[b, tr].index_add_(0, flat, con)
                grad[b, T + t].index_add_(0, flat, -con)
                S[b, tr].index_add_(0, flat, con.abs())
                S[b, T + t].index_add_(0, flat, con.abs())
                M[b, tr] += cnt
                M[b, T + t] += cnt
            if g_next is not None and t < c.nb - 1:
                con = ((invK * on.to(dtype))[:, :, None] * g_next[b, t].reshape(Q, 1, 2).to(dtype)).reshape(-1, 2)
                grad[b, T + t + 1].index_add_(0, flat, con)
                grad[b, T + t].index_add_(0, flat, -con)
                S[b, T + t + 1].index_add_(0, flat, con.abs())
                S[b, T + t].index_add_(0, flat, con.abs())
                M[b, T + t + 1] += cnt
                M[b, T + t] += cnt
    return grad, S, M


def reference(c):
    """Everything the device run of `c` is held against (computed once per case and shared: leave it unchanged)."""
    return _reference(c.name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = case(name)
    idx_all, dist_all = _select(c)
    K = c.K
    idx, dist = idx_all[..., :K], dist_all[..., :K]
    ref = dict(idx=idx, dist=dist, dk=dist[..., K - 1], ik=idx[..., K - 1])
    if idx_all.shape[-1] > K:
        ref['next_idx'] = idx_all[..., K]
        ref['tie'] = dist_all[..., K] == dist_all[..., K - 1]                # a point at exactly the K-th distance that is excluded
    else:
        ref['next_idx'] = None
        ref['tie'] = torch.zeros(idx.shape[:3], dtype=torch.bool)
    ref.update(_values(c, idx))
    g_lut, g_next = c.cotangents()
    grad, S, M = _adjoint(c, idx, g_lut.double(), None if g_next is None else g_next.double())
    gmax = max(float(g_lut.abs().max()), float(g_next.abs().max()) if g_next is not None else 0.0)
    ref['grad'], ref['grad_members'] = grad, M
    ref['grad_allow'] = gamma((n_grad(K, c.norm, c.iwd) + M).double())[..., None] * S + (M.double() * gmax * FAR_QUANTUM)[..., None]
    return ref


def separation(c):
    """The smallest, over all queries, of max over the LUT components (flow_lut, and flow_next where the case has it) of
    |LUT with the K-th neighbour replaced by the (K + 1)-th - LUT| / allowance; inf where n == K."""
    ref = reference(c)
    if ref['next_idx'] is None:
        return float('inf')
    swapped = ref['idx'].clone()
    swapped[..., c.K - 1] = ref['next_idx']
    v = _values(c, swapped)
    def ratio(a, b, allow):                   # (an element that does not move says nothing, whatever its allowance)
        d = (a - b).abs()
        return torch.where(d > 0, d / allow, torch.zeros_like(d))

    r = ratio(v['lut'], ref['lut'], ref['lut_allow']).reshape(c.B, c.nb, c.hq * c.wq, -1).max(-1).values
    if c.has_next:
        rn = ratio(v['nxt'], ref['nxt'], ref['nxt_allow']).reshape(c.B, c.nb - 1, c.hq * c.wq, -1).max(-1).values
        r[:, :c.nb - 1] = torch.maximum(r[:, :c.nb - 1], rn)
    return float(r.min())


# ---- comparator -----------------------------------------------------------------------------------------------------------------
@dataclass
class Result:
    ratio: float
    index: tuple = ()


def compare(got, ref, allow):
    """Largest |got - ref| / allow over all elements; an element with allowance zero must be equal exactly; NaN counts as inf."""
    got, ref, allow = (torch.as_tensor(a).double() for a in (got, ref, allow))
    assert got.shape == ref.shape == allow.shape, (got.shape, ref.shape, allow.shape)
    err = (got - ref).abs()
    ratio = torch.where(allow > 0, err / allow.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    if ratio.numel() == 0:
        return Result(0.0)
    k = int(ratio.argmax())
    return Result(float(ratio.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), ratio.shape)))


RATIOS = {}          # (case, path, output) -> largest ratio seen: the GPU file prints and records them


def _within(c, path, what, got, ref, allow):
    r = compare(got, ref, allow)
    RATIOS[(c.name, path, what)] = r.ratio
    print(f'{c.name} [{path}] {what}: ratio {r.ratio:.3g} at {r.index}', flush=True)
    assert r.ratio <= 1.0, f'{c.name} [{path}] {what}: |got - float64| is {r.ratio:.4g} x the allowance at {r.index}'


def split_state(c, state):
    """knn_state (mpcmax.h:106-109) -> K-th distance [B, nb, Q] float32, K-th index word int32, normaliser, tile maxima
    [B, nb, tiles, 5]."""
    state = torch.as_tensor(state).reshape(-1)
    BQ = c.B * c.nb * c.hq * c.wq
    assert state.numel() == 3 * BQ + c.B * c.nb * num_tiles(c) * KNN_NCLS, state.numel()
    shp = (c.B, c.nb, c.hq * c.wq)
    return (state[:BQ].reshape(shp), state[BQ:2 * BQ].view(torch.int32).reshape(shp), state[2 * BQ:3 * BQ].reshape(shp),
            state[3 * BQ:].reshape(c.B, c.nb, num_tiles(c), KNN_NCLS))


def check_state(c, path, state):
    """The saved state of the forward, the whole interface to the backward."""
    ref = reference(c)
    dk, ikw, norm, tmax = split_state(c, state)
    bad = dk.view(torch.int32) != ref['dk'].view(torch.int32)
    assert not bool(bad.any()), f'{c.name} [{path}] kth distance: {int(bad.sum())} queries differ in bits, first {torch.nonzero(bad)[0].tolist()}'
    bad = (ikw & KNN_IDX_MASK).long() != ref['ik']
    assert not bool(bad.any()), f'{c.name} [{path}] kth index: {int(bad.sum())} queries differ, first {torch.nonzero(bad)[0].tolist()}'
    bad = ref['tie'] & ((ikw & KNN_TIE_FLAG) == 0)
    assert not bool(bad.any()), f'{c.name} [{path}] tie flag: not set at {int(bad.sum())} of {int(ref["tie"].sum())} queries with an excluded tie'
    if c.iwd:
        r = compare(norm, ref['norm'], ref['norm_allow'])
        RATIOS[(c.name, path, 'normaliser')] = r.ratio
        print(f'{c.name} [{path}] normaliser: ratio {r.ratio:.3g} at {r.index}', flush=True)
        assert r.ratio <= 1.0, f'{c.name} [{path}] normaliser: {r.ratio:.4g} x the allowance at {r.index}'
    cls, tile = query_classes(c)
    near = (ikw & KNN_FAR_FLAG) == 0
    for k in range(KNN_NCLS):
        need = torch.zeros(c.B, c.nb, num_tiles(c))
        v = torch.where(near & cls[:, k], ref['dk'], torch.zeros(()))
        need.scatter_reduce_(2, tile.expand(c.B, c.nb, -1), v, 'amax')
        bad = ~(tmax[..., k] >= need)
        assert not bool(bad.any()), (f'{c.name} [{path}] tile maximum: class {k} of tile {torch.nonzero(bad)[0].tolist()} holds '
                                     f'{float(tmax[..., k][bad][0])}, a query of it has {float(need[bad][0])}')
    return int(((ikw & KNN_FAR_FLAG) != 0).sum()), int(((ikw & KNN_TIE_FLAG) != 0).sum())


def check_forward(c, path, lut, nxt):
    ref = reference(c)
    _within(c, path, 'flow_lut', lut, ref['lut'], ref['lut_allow'])
    if c.has_next:
        assert nxt is not None, f'{c.name} [{path}] flow_next: missing'
        _within(c, path, 'flow_next', nxt, ref['nxt'], ref['nxt_allow'])


def check_backward(c, path, grad):
    ref = reference(c)
    nobody = ref['grad_members'] == 0
    got = torch.as_tensor(grad)
    bad = nobody[..., None] & (got != 0)
    assert not bool(bad.any()), f'{c.name} [{path}] zero gradient: {int(bad.sum())} elements of points that are nobody\'s neighbour are not zero'
    _within(c, path, 'grad_traj', got, ref['grad'], ref['grad_allow'])


def check_indices(c, path, idx):
    ref = reference(c)
    bad = (torch.as_tensor(idx).long() != ref['idx']).any(-1)
    assert not bool(bad.any()), f'{c.name} [{path}] neighbour lists: {int(bad.sum())} queries differ, first {torch.nonzero(bad)[0].tolist()}'


# ---- a float32 stand-in of the whole operation, and its mutants -----------------------------------------------------------------------
MUTANTS = {            # mutant -> (the assertion meant to catch it, a case on which it must)
    'ties_to_highest_index': ('kth index', 'lattice_l2_mean'),
    'kth_swapped_in_one_query': ('flow_lut', 'strip_h128_w9'),
    'member_twice_one_dropped': ('flow_lut', 'strip_h128_w9'),
    'backward_strictly_less': ('grad_traj', 'bwd_16x16'),
    'tie_flag_never_set': ('tie flag', 'lattice_l2_mean'),
    'mean_over_K_minus_1': ('flow_lut', 'K_33'),
    'iwd_without_eps': ('normaliser', 'iwd_near_centre'),          # (the first output it reaches; flow_lut is 6 x its allowance off)
    'normaliser_misses_a_term': ('normaliser', 'lattice_l2_iwd'),
    'next_from_same_bin': ('flow_next', 'translate40_l2_mean_next'),
    'tile_max_inner_only': ('tile maximum', 'bwd_17x33'),
    'far_gradient_dropped': ('grad_traj', 'band_translate40'),
}


def standin(c, mutant=None):
    """The operation in float32 with torch's own summation order -> dict(state, lut, nxt, grad, idx).  The neighbour sets are the
    reference's (the kernels rank with the same arithmetic); a mutant breaks one thing."""
    ref = reference(c)
    K, T, Q = c.K, c.T, c.hq * c.wq
    idx, dist = ref['idx'].clone(), ref['dist'].clone()
    tie = ref['tie'].clone()
    if mutant == 'ties_to_highest_index':
        q = c.queries()
        for b in range(c.B):
            for t in range(c.nb):
                d = distances(q, c.traj[b, c.T + t], c.norm)
                o = torch.sort(-torch.arange(c.n).expand_as(d), dim=1, stable=True).indices         # by descending index ...
                o = o.gather(1, torch.sort(d.gather(1, o), dim=1, stable=True).indices)             # ... then, stably, by distance
                idx[b, t], dist[b, t] = o[:, :K], d.gather(1, o[:, :K])
    sum_idx = idx.clone()                       # the sets the sums run over
    if mutant == 'kth_swapped_in_one_query':
        sum_idx[0, 0, Q // 2, K - 1] = ref['next_idx'][0, 0, Q // 2]
    if mutant == 'member_twice_one_dropped':
        sum_idx[0, 0, Q // 2, K - 1] = sum_idx[0, 0, Q // 2, 0]
    tj = c.traj
    lut, nxt, nrm = [], [], []
    kdiv = torch.tensor(float(K - 1 if mutant == 'mean_over_K_minus_1' else K))
    eps = torch.tensor(0.0 if mutant == 'iwd_without_eps' else 1e-9, dtype=torch.float32)
    q = c.queries()
    for b in range(c.B):
        for t in range(c.nb):
            i = sum_idx[b, t]
            f = (tj[b, :T].permute(1, 0, 2) - tj[b, T + t][:, None, :])[i]
            if c.iwd:
                w = 1.0 / (distances(q, tj[b, T + t], c.norm).gather(1, i) + eps)
                ws = w.sum(1)
                lut.append((w[..., None, None] * f).sum(1) / ws[:, None, None])
                nrm.append(ws - w[:, 0] if mutant == 'normaliser_misses_a_term' else ws)
            else:
                lut.append(f.sum(1) / kdiv)
                nrm.append(torch.zeros(Q))
            if c.has_next and t < c.nb - 1:
                src = T + t if mutant == 'next_from_same_bin' else T + t + 1
                nxt.append((tj[b, src] - tj[b, T + t])[i].sum(1) / torch.tensor(float(K)))
    lut = torch.stack(lut).reshape(c.B, c.nb, c.hq, c.wq, T, 2)
    nxt = torch.stack(nxt).reshape(c.B, c.nb - 1, c.hq, c.wq, 1, 2) if c.has_next else None
    dk, ik = dist[..., K - 1], idx[..., K - 1]
    far = (dk > far_limit(c)) if strip_usable(c) else torch.zeros_like(tie)
    word = ik.int() | torch.where(tie & (mutant != 'tie_flag_never_set'), KNN_TIE_FLAG, 0).int() | torch.where(far, KNN_FAR_FLAG, 0).int()
    cls, tile = query_classes(c)
    tmax = torch.zeros(c.B, c.nb, num_tiles(c), KNN_NCLS)
    for k in range(KNN_NCLS if mutant != 'tile_max_inner_only' else 1):
        v = torch.where(~far & cls[:, k], dk, torch.zeros(()))
        tmax[..., k].scatter_reduce_(2, tile.expand(c.B, c.nb, -1), v, 'amax')
    state = torch.cat((dk.reshape(-1), word.reshape(-1).view(torch.float32), torch.stack(nrm).reshape(-1), tmax.reshape(-1)))
    member = None
    if mutant == 'backward_strictly_less':
        member = dist < dk[..., None]
    if mutant == 'far_gradient_dropped':
        member = (~far)[..., None].expand_as(idx)
    g_lut, g_next = c.cotangents()
    grad, _, _ = _adjoint(c, idx, g_lut, g_next, dtype=torch.float32, member=member)
    return dict(state=state, lut=lut, nxt=nxt, grad=grad, idx=idx)


def check_all(c, path, out):
    """Every assertion of the GPU file on one set of outputs (the host file runs the stand-in and its mutants through it)."""
    check_state(c, path, out['state'])
    check_forward(c, path, out['lut'], out['nxt'])
    check_backward(c, path, out['grad'])
    check_indices(c, path, out['idx'])


# ---- geometries: the mid-time rows [B, nb, n, 2] -----------------------------------------------------------------------------------
def tile_centres(H, W, patch):
    """One point per patch x patch tile at offset patch // 2 (utils/trajectories.py: get_optical_flow_tile_mask) -> [n, 2]."""
    gy, gx = torch.meshgrid(torch.arange(patch // 2, H, patch, dtype=torch.float32),
                            torch.arange(patch // 2, W, patch, dtype=torch.float32), indexing='ij')
    return torch.stack((gy, gx), -1).reshape(-1, 2)


def g_lattice(H, W, patch, B=1, nb=3):
    """The `zero` family of utils/synth.py: the exact lattice in every bin."""
    return tile_centres(H, W, patch).expand(B, nb, -1, 2).clone()


def g_jitter(H, W, patch, B=1, nb=2, seed=0, amp=1.5):
    """The lattice with every point moved by up to `amp` px, anew in every bin: no ties, every cell populated."""
    g = torch.Generator().manual_seed(seed)
    p = tile_centres(H, W, patch)
    return p + (torch.rand(B, nb, p.shape[0], 2, generator=g) * 2 - 1) * amp


def g_uniform(H, W, n, B=1, nb=1, seed=0, ext=4.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, nb, n, 2, generator=g) * torch.tensor([H + 2 * ext, W + 2 * ext]) - ext


def g_family(H, W, patch, family, B=1, nb=3, seed=0):
    from motionpriorcmax_amd.utils import synth
    return synth.synth_trajectories(B, 3, nb, (H, W), patch, family, seed=seed)[0][:, 1:].contiguous()


def cell_of(v, sp):
    """cell_of, knn_device.h:137-141 without the clamp: cell c covers [c sp - 0.5, (c + 1) sp - 0.5)."""
    return torch.floor((v + 0.5) / sp)


def with_piles(mid, sp, cells, count, seed):
    """Exactly `count` points in each of `cells` (cy, cx) in every (sample, bin): the points that lie in a cell stay (up to `count`;
    any more move one cell to the right), the rest are taken from outside the cells at an even stride through the index range, and
    all get seeded places inside the cell."""
    g = torch.Generator().manual_seed(seed)
    out = mid.clone()
    for b in range(mid.shape[0]):
        for t in range(mid.shape[1]):
            p = out[b, t]
            cyx = torch.stack((cell_of(p[:, 0], sp), cell_of(p[:, 1], sp)), 1)
            inside = [(cyx[:, 0] == cy) & (cyx[:, 1] == cx) for cy, cx in cells]
            free = torch.nonzero(~torch.stack(inside).any(0)).flatten().tolist()
            for (cy, cx), ins in zip(cells, inside):
                have = torch.nonzero(ins).flatten().tolist()
                for i in have[count:]:
                    p[i, 1] = p[i, 1] + sp
                keep = have[:count]
                need = count - len(keep)
                if need > 0:
                    stride = max(1, len(free) // need)
                    got = free[::stride][:need]
                    free = [i for i in free if i not in set(got)]
                    keep = keep + got
                assert len(keep) == count
                lo = torch.tensor([cy * sp - 0.5, cx * sp - 0.5])
                p[keep] = lo + 0.125 + torch.rand(count, 2, generator=g) * (sp - 0.25)
    return out


IWD_KEEP_OFF = 0.7


def keep_off_centres(mid, sp, r=IWD_KEEP_OFF):
    """Every point nearer than r px to a cell centre is moved straight away from it to r px (a point ON a centre: along x).  An
    'iwd' weight 1 / (d + 1e-9) of a point that close drowns the K-th neighbour's, and no exchange of neighbours would show in
    flow_lut; the lattices (0.707 px from the nearest centre) are left as they are."""
    off = sp / 2 - 0.5
    centre = torch.round((mid - off) / sp) * sp + off
    v = mid - centre
    d = v.norm(dim=-1, keepdim=True)
    unit = torch.where(d > 0, v / d.clamp_min(1e-30), torch.tensor([0.0, 1.0]).expand_as(v))
    return torch.where(d < r, centre + unit * (r * 1.001), mid)


def make(name, mid, H, W, sp=4, K=32, norm='l2', scheme='mean', want_next=False, T=1, seed=1, expect=(), note=''):
    """The case of mid-time rows `mid` [B, nb, n, 2]: reference rows = mid row 0 + e, e uniform in [-8, 8]^2 per point and row.
    'iwd' cases keep their points off the cell centres (keep_off_centres)."""
    g = torch.Generator().manual_seed(1000 + seed)
    mid = mid.float()
    if scheme == 'iwd' and K > 1:
        mid = keep_off_centres(mid, sp)
    B, nb, n, _ = mid.shape
    ref = torch.stack([mid[:, 0] + (torch.rand(B, n, 2, generator=g) * 16 - 8) for _ in range(T)], 1)
    return Case(name=name, H=H, W=W, sp=sp, K=K, norm=norm, scheme=scheme, want_next=want_next, T=T,
                traj=torch.cat((ref, mid), 1).contiguous(), expect=tuple(expect), note=note)


# what the device run must show (tests/test_gpu_knn_cases.py: routes()).  STRIP: the strip kernel and the tile gather with its far
# list; QUERY: the general tile kernel forward
STRIP = (('k_knn_strip', '>', 0), ('k_knn_query', '==', 0), ('k_knn_bwd_tile', '>', 0), ('k_knn_bwd_far', '>', 0))
QUERY = (('k_knn_strip', '==', 0), ('k_knn_query', '>', 0))
LDS_SORT = (('k_knn_bucket', '>', 0), ('k_knn_bucket_count', '==', 0))
DIRECT, BINS = (('k_knn_bwd_combine_direct', '>', 0),), (('k_knn_bwd_combine_bins', '>', 0),)


def _grid(hq, wq, sp=4):
    return hq * sp, wq * sp


def _c_strip(name, hq, wq):
    H, W = _grid(hq, wq)
    return make(name, g_jitter(H, W, 4, nb=2, seed=hq * 100 + wq), H, W, expect=STRIP + LDS_SORT + DIRECT)


def _c_bwd(name, hq, wq):
    H, W = _grid(hq, wq)
    return make(name, g_jitter(H, W, 4, nb=3, seed=hq * 100 + wq), H, W, want_next=True, expect=STRIP + BINS)


def _c_tiny(name, hq, wq, n=None):
    H, W = _grid(hq, wq)
    mid = g_jitter(H, W, 4, nb=2, seed=hq * 100 + wq) if n is None else g_uniform(H, W, n, nb=2, seed=7, ext=8.0)
    return make(name, mid, H, W, expect=QUERY + (('k_knn_bwd_tile', '>', 0),))


def _c_K(name, K, norm='l2', hq=24, wq=24, n=None):
    H, W = _grid(hq, wq)
    mid = g_jitter(H, W, 4, nb=2, seed=K) if n is None else g_uniform(H, W, n, nb=2, seed=K, ext=2.0)
    c = make(name, mid, H, W, K=K, norm=norm)
    c.expect = (STRIP if strip_usable(c) else QUERY) + (('k_knn_bwd_tile', '>', 0),)
    return c


def _eseed(norm, scheme):
    """Seed of the reference rows' offsets: 'iwd' with 'l2' gives its K-th neighbour the smallest share of a sum, and of the seeds
    1 .. 12 only 10 keeps every query of both 40 x 48 geometries above SEPARATION (22 and 28; tests/test_knn_cases_host.py)."""
    return 10 if (norm, scheme) == ('l2', 'iwd') else 1


def _c_lattice(name, sp=4, patch=4, norm='l2', scheme='mean', want_next=False, expect=None):
    H, W = 160, 192
    c = make(name, g_lattice(H, W, patch), H, W, sp=sp, norm=norm, scheme=scheme, want_next=want_next, seed=_eseed(norm, scheme))
    c.expect = expect if expect is not None else (STRIP if strip_usable(c) else QUERY) + (('ref_ties', '>', 1000),)
    if (sp, patch) == (2, 4):              # a quarter of the density: every strip has far queries, and the far items leave a late list
        c.expect += FAR + FAR_PASS + (('late', '>', 0),)
    return c


def _c_one_spot(name):
    H, W = _grid(8, 8)
    mid = torch.full((1, 2, 64, 2), 13.25)
    mid[:, 1] = torch.tensor([20.0, 7.5])
    return make(name, mid, H, W, expect=(('ref_ties', '==', 128),))


def _c_pairs(name):
    import knn_wide_cases as KW
    H, W = KW.H, KW.W
    mid = g_jitter(H, W, 4, nb=2, seed=3)
    c = make(name, mid, H, W, expect=STRIP)
    c.traj[:, 1:] = KW.with_duplicates(c.traj[:, 1:], KW.chunk_starts(c.n, 100))
    return c


def _c_near_centre(name):
    """'iwd' where the 1e-9 matters: two points 2^-16 and 2^-13 px from a query centre (bin 0 only; both offsets are exact in
    float32 on this grid; weights 0.81e9 and 0.63e8 with the 1e-9, 4.3e9 and 0.67e8 without).  These weights drown the K-th neighbour's in flow_lut, so the case carries flow_next --
    always a mean -- which keeps every neighbour set visible."""
    H, W = _grid(16, 16)
    mid = g_jitter(H, W, 4, nb=2, seed=11)
    c = make(name, mid, H, W, scheme='iwd', want_next=True, expect=STRIP)
    q = c.queries()
    for j, qi in enumerate((17, 40, 100, 135, 200, 238)):
        c.traj[0, 1, 2 * j] = q[qi] + torch.tensor([0.0, 2.0 ** -16])
        c.traj[0, 1, 2 * j + 1] = q[qi] + torch.tensor([2.0 ** -13, 0.0])
    return c


CELLS = {'inner': (16, 16), 'border': (0, 5), 'ring': (-KNN_MARGIN, 10)}


def _c_pile(name, count):
    H, W = _grid(32, 32)
    mid = with_piles(g_jitter(H, W, 4, nb=2, seed=count), 4, list(CELLS.values()), count, seed=count * 10)
    return make(name, mid, H, W, expect=STRIP)


def _c_margin(name):
    """Points at -7, -7.5 and -8 cells and at hq + 6, + 7 and + 8 cells, along both axes (the margin ring and what is clamped into
    it), on top of a jittered lattice."""
    hq, wq = 24, 24
    H, W = _grid(hq, wq)
    mid = g_jitter(H, W, 4, nb=2, seed=5)
    g = torch.Generator().manual_seed(6)
    k = 0
    for cells in (-7.0, -7.5, -8.0, hq + 6.0, hq + 7.0, hq + 8.0):
        for axis in (0, 1):
            for _ in range(12):
                along = float(torch.rand(1, generator=g)) * (H + 40) - 20
                p = torch.tensor([cells * 4 + 1.5, along]) if axis == 0 else torch.tensor([along, cells * 4 + 1.5])
                mid[:, :, k] = p
                k += 1
    return make(name, mid, H, W, expect=STRIP)


def _c_bin_outside(name):
    H, W = _grid(24, 24)
    mid = g_jitter(H, W, 4, nb=2, seed=8)
    mid[:, 1, :, 1] += W + 500.0
    return make(name, mid, H, W, expect=STRIP + (('far_flags', '>', 0),))


def _c_family(name, family, B=1, nb=3, expect=None, norm='l2', scheme='mean', want_next=False, seed=31):
    H, W = 160, 192
    c = make(name, g_family(H, W, 4, family, B=B, nb=nb, seed=seed), H, W, norm=norm, scheme=scheme, want_next=want_next,
             seed=_eseed(norm, scheme))
    c.expect = expect if expect is not None else ((STRIP + FAR + SMALL_TAIL) if strip_usable(c) else QUERY)
    return c


def _c_crowded_stripe(name):
    """Staging overflow: the lattice with two more points in every tile of six columns -- three times the density in a strip and
    its halo (a wider stripe lifts the mean density beyond what the strip kernel takes, strip_geometry, knn_strip.hip:1342).  There a query's own
    radius is 2 cells (75 points in its square, within the 96 slots), so the strip stages 6 columns x 40 rows x 3 = 720 points
    where the area holds 1.15 x the mean density of 1.25 plus 32: 592 (knn_strip.hip:1343-1345)."""
    H, W = 160, 192
    p = tile_centres(H, W, 4)
    inside = (p[:, 1] >= 80) & (p[:, 1] < 104)
    parts = [g_jitter(H, W, 4, nb=2, seed=14)] + [g_jitter(H, W, 4, nb=2, seed=s)[:, :, inside] for s in (15, 16)]
    return make(name, torch.cat(parts, 2), H, W, expect=STRIP + (('retry', '>', 0),))


def _c_band_both_sides(name):
    """A band of 14 cell rows without a point, dense on both of its sides."""
    H, W = 160, 192
    mid = g_jitter(H, W, 4, nb=2, seed=9)
    y = mid[..., 0]
    inside = (y > 50) & (y < 106)
    mid[..., 0] = torch.where(inside, torch.where(y < 78, 50 - (y - 50) * 0.1, 106 + (106 - y) * 0.1), y)
    return make(name, mid, H, W, expect=STRIP + FAR + SMALL_TAIL)


def _c_deep_band(name):
    """A query deep in a band of a dense set: patch 2, K 64."""
    H, W = 160, 192
    mid = g_family(H, W, 2, 'translate40', nb=1, seed=31)
    c = make(name, mid, H, W, K=64)
    c.expect = (STRIP if strip_usable(c) else QUERY)
    return c


def _c_plan(name, B, nb):
    H, W = _grid(16, 16)
    c = make(name, g_jitter(H, W, 4, B=B, nb=nb, seed=B * nb), H, W)
    S, big = sort_plan(c)
    c.expect = STRIP + LDS_SORT + (('k_knn_sat', '>' if S != 1 else '==', 0),)
    return c


def _c_n(name, n):
    H, W = _grid(32, 32)
    return make(name, g_uniform(H, W, n, seed=n), H, W, expect=QUERY + LDS_SORT)


def _c_global_sort(name):
    H, W = 372, 386
    c = make(name, g_jitter(H, W, 8, nb=1, seed=12, amp=3.0), H, W, sp=2)
    assert sort_plan(c)[1]
    c.expect = QUERY + (('k_knn_bucket', '==', 0), ('k_knn_bucket_count', '>', 0))
    return c


def _c_T2(name, hq, wq, norm='l2', scheme='mean', want_next=True, T=2):
    """num_tref > 1: the general tile kernel forward and the general gather (k_knn_bwd_points, k_knn_bwd_combine), three bins."""
    H, W = _grid(hq, wq)
    return make(name, g_jitter(H, W, 4, nb=3, seed=hq), H, W, norm=norm, scheme=scheme, want_next=want_next, T=T,
                expect=QUERY + (('k_knn_bwd_points', '>', 0), ('k_knn_bwd_combine', '>', 0)))


FAR = (('far_flags', '>', 0),)
# the tail launch's two ways: few marked queries -- its fallback workgroups take them from the marked list, no far items, no strip
# workgroup counts itself done --, or more than KS_FORWARD_MAX: the far items
SMALL_TAIL = (('marked', '>', 0), ('marked', '<=', KS_FORWARD_MAX), ('done', '==', 0))
FAR_PASS = (('marked', '>', KS_FORWARD_MAX), ('done', '>', 0))
CASES = {}
for _h in (127, 128, 129):
    CASES[f'strip_h{_h}_w9'] = (_c_strip, (_h, 9))
CASES['strip_h8_w8'] = (_c_strip, (8, 8))
for _h, _w in ((15, 17), (16, 16), (17, 33), (33, 15)):
    CASES[f'bwd_{_h}x{_w}'] = (_c_bwd, (_h, _w))
CASES['tiny_1x1_n_eq_K'] = (_c_tiny, (1, 1, 32))
CASES['tiny_7x9'] = (_c_tiny, (7, 9))
CASES['tiny_3x40'] = (_c_tiny, (3, 40))
for _k in (1, 2, 31, 33, 64, 96, 97):
    CASES[f'K_{_k}'] = (_c_K, (_k,))
CASES['K_128_l1'] = (_c_K, (128, 'l1'))
CASES['K_129_l1'] = (_c_K, (129, 'l1'))
CASES['K_eq_n_12x12'] = (_c_K, (32, 'l2', 12, 12, 32))
for _norm in ('l2', 'l1'):
    for _scheme in ('mean', 'iwd'):
        for _next in (False, True):
            _sfx = f'{_norm}_{_scheme}' + ('_next' if _next else '')
            CASES[f'lattice_{_sfx}'] = (_c_lattice, (4, 4, _norm, _scheme, _next))
            CASES[f'translate40_{_sfx}'] = (_c_family, ('translate40', 1, 3, None, _norm, _scheme, _next))
CASES['lattice_sp2_patch4'] = (_c_lattice, (2, 4))
CASES['lattice_sp4_patch2'] = (_c_lattice, (4, 2))
CASES['dup_one_spot'] = (_c_one_spot, ())
CASES['dup_pairs'] = (_c_pairs, ())
CASES['iwd_near_centre'] = (_c_near_centre, ())
for _p in (6, 7, 16, 17, 128, 129):
    CASES[f'pile_{_p}'] = (_c_pile, (_p,))
CASES['margin_points'] = (_c_margin, ())
CASES['bin_outside'] = (_c_bin_outside, ())
CASES['band_translate40'] = (_c_family, ('translate40', 3, 3, STRIP + FAR + FAR_PASS))
# (translate10 empties 2.5 cell rows of this grid: its few stray queries go on the fail list and nothing is marked; the marked list
# with at most 1 024 entries is the route of translate40_* at B = 1, margin_points, bin_outside and pile_128 / 129)
CASES['band_translate10'] = (_c_family, ('translate10', 1, 1, STRIP + (('fails', '>', 0), ('marked', '<=', KS_FORWARD_MAX), ('done', '==', 0))))
# (a 40 x 48 grid under diverge-45 does not overflow the staging area -- the emptied border rows make room for the packed middle;
# band_crowded_stripe does -- but crowds cells beyond the fast path's slots: reason 1)
CASES['band_diverge-45'] = (_c_family, ('diverge-45', 1, 3, STRIP + FAR + (('why1', '>', 0),)))
CASES['band_diverge+45'] = (_c_family, ('diverge+45', 1, 3, STRIP + (('why0', '>', 0),)))
CASES['band_crowded_stripe'] = (_c_crowded_stripe, ())
CASES['band_both_sides'] = (_c_band_both_sides, ())
CASES['deep_band_dense'] = (_c_deep_band, ())
for _b, _nb in ((1, 1), (4, 16), (10, 10), (9, 15)):
    CASES[f'plan_{_b * _nb}'] = (_c_plan, (_b, _nb))
for _n in (8192, 8193, 16384, 16385, 20480, 20481, 24576, 24577):
    CASES[f'n_{_n}'] = (_c_n, (_n,))
CASES['global_sort'] = (_c_global_sort, ())
CASES['T2_17x33'] = (_c_T2, (17, 33))
CASES['T2_40x48'] = (_c_T2, (40, 48))
# (the 'iwd' weight of the general gather, and its flow_next partials read as zeros; three reference times through both loops of the
# combine on a grid under one tile in height and just over one in width)
CASES['T2_17x33_iwd_l1'] = (_c_T2, (17, 33, 'l1', 'iwd', False))
CASES['T3_15x17'] = (_c_T2, (15, 17, 'l2', 'mean', False, 3))

# one case per route also goes through ops.KnnLutFn
FN_CASES = ('strip_h129_w9', 'bwd_17x33', 'tiny_7x9', 'band_translate40', 'band_translate10', 'global_sort', 'T2_17x33', 'lattice_l1_iwd_next')


@functools.lru_cache(maxsize=None)
def case(name):
    fn, args = CASES[name]
    return fn(name, *args)
