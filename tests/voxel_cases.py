"""Named edge cases of the voxel-grid builder (csrc/voxel.hip), the geometry that proves each reaches its route, and the rule by
which a device grid is compared with the float64 oracle.  A helper module (no fixtures): tests/test_voxel_cases_host.py checks
the cases on the CPU, tests/test_gpu_voxel_cases.py runs them on the device, tools/fuzz_voxel.py draws random ones.

The bound, for every output tensor X (norm / quantile applied):

    max |X_gpu - X_64| <= max(4 err32, 2^-22 max |X_64|) + T 2^-30 m

err32 = max |oracle_fp32 - oracle_fp64| on the CPU (never taken from the kernel), T = the most taps on one entry (each tap is
truncated to a multiple of 2^-30 by mpc_to_fixed), m = the multiplier the oracle applies last (1, 1 / std, 1 / max).

Two caps, conditions on the INPUTS: no entry has 0 < |raw_64| <= the raw bound (such an entry may truncate to 0 on the device and
drop out of the statistics), fp32 and fp64 agree on which entries are non-zero; and entries that are zero in fp64 are +-0 on the
device.  Nothing is excused."""
import functools
import os

import numpy as np
import torch

from oracle import voxel_oracle as V

VOX_STRIP_KB = 75            # csrc/tuning.h
VOX_PER_THREAD = 2           # csrc/voxel.hip
VOX_QBINS = 2048
NORMS = (None, 'mean_std', 'max')


# ---- geometry: vox_layout / sb_layout restated -------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def _align(n, a=256):
    return _cdiv(n, a) * a


def vox_geometry(shape, N, B=1):
    """SR rows per strip, NS strips, nloc buckets per sample, cap records per bucket, spill / chunk capacities and the workspace
    bytes of mpc_voxel_grid for B samples of N events (asserted equal to mpc_voxel_workspace_bytes for every case)."""
    C, H, W = shape
    SR = (VOX_STRIP_KB * 1024) // (W * 8)
    if SR < 1:
        SR = (150 * 1024) // (W * 8)
    SR = min(SR, H)
    NS = _cdiv(H, SR)
    SR = _cdiv(H, NS)
    nloc = C * NS
    B1 = max(B, 1)
    NBk = B * nloc
    cap = max(4 * _cdiv(2 * N, nloc), 4096)
    cap = max(min(cap, 2 * N), 1)
    per_event, wg_events = 4, 256 * VOX_PER_THREAD
    spcap = max(per_event * N, 1)
    chcap = _cdiv(max(N, 1), wg_events) * min(nloc, wg_events * per_event)
    ws = (_align((NBk + 2 * B1 + 8) * 4) + _align(NBk * cap * 16 + 16) + _align(B1 * spcap * 16 + 16) + _align(B1 * chcap * 16 + 16)
          + _align(B1 * 256 * 4 * 8) + _align(max(NBk, 1) * 4 * 8) + _align(B1 * 16) + _align(B1 * VOX_QBINS * 4) + _align(B1 * 32))
    return dict(SR=SR, NS=NS, nloc=nloc, cap=cap, spcap=spcap, chcap=chcap, lds=SR * W * 8, ws=ws)


def bucket_fills(x, y, t, shape, SR, NS):
    """Records per (channel, strip) bucket as k_vox_bin makes them: [C, NS] int64.  An event whose two rows lie in one strip
    leaves one record per channel there, in two strips one in each."""
    C, H, W = shape
    fills = torch.zeros(C, NS, dtype=torch.int64)
    if x.numel() == 0:
        return fills
    tn = (C - 1) * (t - t[0]) / (t[-1] - t[0])
    t0 = torch.where(torch.isfinite(tn), tn.clamp(-4.0, C + 4.0), torch.full_like(tn, -4.0)).int()
    x0 = torch.nan_to_num(x, nan=-8.0).clamp(-8.0, W + 8.0).int()
    y0 = torch.nan_to_num(y, nan=-8.0).clamp(-8.0, H + 8.0).int()
    on = (x0 + 1 >= 0) & (x0 < W)
    for dt in (0, 1):
        tl = t0 + dt
        okt = on & (tl >= 0) & (tl < C)
        prev = torch.full_like(y0, -1)
        for dy in (0, 1):
            yl = y0 + dy
            st = torch.div(yl, SR, rounding_mode='floor')
            ok = okt & (yl >= 0) & (yl < H) & (st != prev)
            prev = torch.where(okt & (yl >= 0) & (yl < H), st, prev)
            fills.view(-1).put_((tl.long() * NS + st.long())[ok], torch.ones(int(ok.sum()), dtype=torch.int64), accumulate=True)
    return fills


# ---- the cases ----------------------------------------------------------------------------------------------------------
class Case:
    """samples: list of (x, y, t, p) fp32 tensors; N: rows of the padded batch; counts: what the kernel is told (None: the true
    lengths); combos: the (norm, quantile) pairs the case is run with; expect: per-sample events the grid must equal (None: its
    own events) -- the non-finite case is judged against the events WITHOUT its bad rows."""

    def __init__(self, name, shape, samples, combos, N=None, counts=None, expect=None):
        self.name, self.shape, self.samples, self.combos = name, tuple(shape), samples, tuple(combos)
        self.N = N if N is not None else max(max(s[0].numel() for s in samples), 1)
        self.counts = counts if counts is not None else [s[0].numel() for s in samples]
        self.expect = expect if expect is not None else samples

    @property
    def B(self):
        return len(self.samples)

    def batch(self):
        """-> ev [B, N, 4] fp32 (x, y, t, p), counts [B] int32.  The rows past a sample's length hold a valid event in the middle of
        the sensor: a kernel that reads them shows it."""
        C, H, W = self.shape
        ev = torch.empty(self.B, self.N, 4)
        ev[..., 0], ev[..., 1], ev[..., 2], ev[..., 3] = 0.4 * W, 0.4 * H, 0.5, 1.0
        for b, s in enumerate(self.samples):
            n = s[0].numel()
            if n:
                ev[b, :n] = torch.stack([v.float() for v in s], -1)
        return ev, torch.tensor(self.counts, dtype=torch.int32)

    def geometry(self):
        return vox_geometry(self.shape, self.N, self.B)

    def fills(self, b):
        g = self.geometry()
        x, y, t, _ = self.samples[b]
        return bucket_fills(x, y, t, self.shape, g['SR'], g['NS'])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def frac(n, g, lo=0.03, hi=0.97):
    """Fractional parts away from 0 and 1: the smallest tap weight stays far above the bound (cap 1)."""
    return lo + (hi - lo) * torch.rand(n, generator=g)


def coords(n, lo, hi, g):
    """Coordinates with integer part uniform in [lo, hi) and a fraction of `frac`."""
    return torch.randint(lo, hi, (n,), generator=g).float() + frac(n, g)


def uniform_events(n, shape, g, ylo=None, yhi=None):
    C, H, W = shape
    x = coords(n, -2, W + 1, g)
    y = coords(n, -2 if ylo is None else ylo, H + 1 if yhi is None else yhi, g)
    # t_norm = (C - 1) t: an integer channel plus a fraction of `frac`, sorted, first and last pinned to 0 and 1
    if C > 1:
        t = torch.sort((torch.randint(0, C - 1, (n,), generator=g).float() + frac(n, g)) / (C - 1)).values
    else:
        t = torch.sort(torch.rand(n, generator=g)).values
    t[0], t[-1] = 0.0, 1.0
    p = (torch.rand(n, generator=g) > 0.5).float()
    return x, y, t, p


ALL = tuple((n, q) for n in NORMS for q in (0.0, 0.05))
PLAIN = tuple((n, 0.0) for n in NORMS)


def case_spill():
    """(5, 10, 2400), B = 2, 6000 + 6000: rows 4..7 (one strip), t_norm in (1, 2): two buckets per sample far past cap 4096."""
    shape, out = (5, 10, 2400), []
    for seed in (101, 102):
        g = gen(seed)
        n = 6000
        x = coords(n, -2, shape[2] + 1, g)
        y = coords(n, 4, 7, g)
        t = torch.sort((1.0 + frac(n, g)) / 4.0).values
        t[0], t[-1] = 0.0, 1.0
        p = (torch.rand(n, generator=g) > 0.5).float()
        out.append((x, y, t, p))
    return Case('spill', shape, out, PLAIN + (('mean_std', 0.05),))


def case_short_strip():
    """(3, 10, 2400): SR 4, NS 3, rows 4 / 4 / 2; events with y in [3, 4) and [7, 8) have their two rows in different strips."""
    shape = (3, 10, 2400)
    g = gen(111)
    x, y, t, p = uniform_events(4000, shape, g)
    y[1000:1500] = 3.0 + frac(500, g)
    y[1500:2000] = 7.0 + frac(500, g)
    y[2000:2300] = 9.0 + frac(300, g)             # the last row of the short strip, its second row off the sensor
    return Case('short_strip', shape, [(x, y, t, p)], ALL)


def case_wide():
    """(2, 3, 12000): 75 KB hold no row of 96 000 bytes, SR falls back to 1 (150 KB budget), NS 3."""
    shape = (2, 3, 12000)
    return Case('wide', shape, [uniform_events(5000, shape, gen(121))], ALL)


def case_tiny(shape, n, seed):
    g = gen(seed)
    C, H, W = shape
    x = coords(n, -1, W, g) if W > 1 else -0.9 + 1.8 * torch.rand(n, generator=g)
    y = coords(n, -1, H, g) if H > 1 else -0.9 + 1.8 * torch.rand(n, generator=g)
    _, _, t, p = uniform_events(n, shape, g)
    return Case('tiny_%dx%dx%d' % shape, shape, [(x, y, t, p)], tuple((nm, q) for nm in NORMS for q in (0.0, 0.05, 0.125)))


def case_integer_ties(seed=134):
    """(5, 24, 32), 3000 events with integer x, y and 4 t: every event is one tap of +-1; |v| takes five values, 2047 entries are 0."""
    shape = (5, 24, 32)
    g = gen(seed)
    n = 3000
    x = torch.randint(0, shape[2], (n,), generator=g).float()
    y = torch.randint(0, shape[1], (n,), generator=g).float()
    t = torch.sort(torch.randint(0, 5, (n,), generator=g).float() / 4.0).values
    t[0], t[-1] = 0.0, 1.0
    p = (torch.rand(n, generator=g) > 0.5).float()
    return Case('integer_ties', shape, [(x, y, t, p)], tuple((nm, q) for nm in NORMS for q in (0.0, 0.02, 0.05, 0.1, 0.14)))


def case_sparse(seed=141):
    """(5, 24, 32), 50 events: fewer than a tenth of the entries are touched, the 0.9 quantile of |grid| is 0."""
    shape = (5, 24, 32)
    return Case('sparse', shape, [uniform_events(50, shape, gen(seed))], tuple((nm, 0.1) for nm in NORMS) + PLAIN)


def case_time():
    """Unsorted times, some before t[0] and after t[-1] (first and last rows pinned): t_norm from -1.67 to C - 1 + 1.67, negative
    weights on channel 1, `(int)` truncation towards zero."""
    shape = (4, 12, 16)
    g = gen(151)
    n = 200
    x, y, _, p = uniform_events(n, shape, g)
    # t_norm = 3 (t - 0.25) / 0.5: integer part in [-2, 5), fraction of `frac`, shuffled
    tn = torch.randint(-2, 5, (n,), generator=g).float() + frac(n, g)
    t = 0.25 + tn / 6.0
    t[0], t[-1] = 0.25, 0.75
    return Case('time', shape, [(x, y, t, p)], ALL)


def case_ragged():
    """(5, 24, 32), B = 4: counts [0, N, 1, N + 5]; the kernel clamps the last to N, an empty and a one-event sample give zeros."""
    shape = (5, 24, 32)
    n = 400
    full = [uniform_events(n, shape, gen(161 + b)) for b in range(2)]
    one = tuple(v[:1].clone() for v in uniform_events(4, shape, gen(165)))
    empty = tuple(torch.zeros(0) for _ in range(4))
    return Case('ragged', shape, [empty, full[0], one, full[1]], ALL, N=n, counts=[0, n, 1, n + 5])


BAD_XY = (float('nan'), float('inf'), float('-inf'), 1e10, -1e10, -9.0)


def case_nonfinite():
    """x or y NaN, +-inf, +-1e10, -9, W + 9 / H + 9 at middle rows: the grid equals the one built without those rows."""
    shape = (3, 12, 16)
    g = gen(171)
    n = 120
    x, y, t, p = uniform_events(n, shape, g)
    bad = torch.zeros(n, dtype=torch.bool)
    xb, yb = x.clone(), y.clone()
    vals_x, vals_y = BAD_XY + (shape[2] + 9.0,), BAD_XY + (shape[1] + 9.0,)
    for i, v in enumerate(vals_x):
        xb[10 + i], bad[10 + i] = v, True
    for i, v in enumerate(vals_y):
        yb[40 + i], bad[40 + i] = v, True
    xb[70], yb[70], bad[70] = float('nan'), float('inf'), True
    keep = ~bad
    return Case('nonfinite', shape, [(xb, yb, t, p)], ALL, expect=[(x[keep], y[keep], t[keep], p[keep])])


def case_all_equal():
    """(5, 12, 16): 40 events at distinct integer pixels, t = 1 + 0.7 / (C - 1), between two off-sensor events at t = 0 and 1:
    40 equal entries of about 0.3 in the last channel.  The reference's std is exactly 0: only the mean is subtracted."""
    shape = (5, 12, 16)
    g = gen(181)
    pix = torch.randperm(shape[1] * shape[2], generator=g)[:40]
    x = torch.cat((torch.tensor([-5.0]), (pix % shape[2]).float(), torch.tensor([-5.0])))
    y = torch.cat((torch.tensor([3.0]), (pix // shape[2]).float(), torch.tensor([3.0])))
    t = torch.cat((torch.tensor([0.0]), torch.full((40,), 1.0 + 0.7 / 4), torch.tensor([1.0])))
    return Case('all_equal', shape, [(x, y, t, torch.ones(42))], (('mean_std', 0.0),))


def case_zero_span():
    """First and last time equal, the middle ones not: t_norm is 0 / 0 at the ends and +-inf between.  The reference's int
    conversion masks every tap: an all-zero, finite grid."""
    shape = (3, 6, 8)
    f = lambda *v: torch.tensor(v, dtype=torch.float32)          # noqa: E731
    return Case('zero_span', shape, [(f(2.5, 4.25, 1.75, 6.5), f(3.25, 1.5, 2.75, 4.5), f(0.5, 0.2, 0.9, 0.5), f(1, 0, 1, 1))], PLAIN)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [case_spill(), case_short_strip(), case_wide(), case_tiny((1, 1, 1), 2, 191), case_tiny((2, 1, 9), 37, 192),
          case_tiny((3, 5, 7), 300, 193), case_integer_ties(), case_sparse(), case_time(), case_ragged(), case_nonfinite(),
          case_all_equal(), case_zero_span()]
    return {c.name: c for c in cs}


CASE_NAMES = ('spill', 'short_strip', 'wide', 'tiny_1x1x1', 'tiny_2x1x9', 'tiny_3x5x7', 'integer_ties', 'sparse', 'time', 'ragged',
              'nonfinite', 'all_equal', 'zero_span')


def case_params():
    """(case, norm, quantile) for pytest.mark.parametrize."""
    return [(n, nm, q) for n in CASE_NAMES for nm, q in cases()[n].combos]


# ---- the comparison -------------------------------------------------------------------------------------------------------
def oracles(events, shape, norm, q):
    """-> dict: g64, taps, raw64, m (oracle.voxel_oracle.voxel_grid64), g32 and raw32 (voxel_grid, the pinned fp32 oracle)."""
    x, y, t, p = events
    g64, taps, raw64, m = V.voxel_grid64(x, y, t, p, shape, norm, q)
    if x.numel() == 0:
        g32 = raw32 = torch.zeros(shape)
    else:
        g32 = V.voxel_grid(x, y, t, p, shape, norm, q)
        raw32 = g32 if (norm is None and q == 0) else V.voxel_grid(x, y, t, p, shape, None, 0.0)
    return dict(g64=g64, taps=taps, raw64=raw64, m=m, g32=g32, raw32=raw32)


@functools.lru_cache(maxsize=None)
def expected(name, norm, q):
    """The oracles of every sample of a named case, computed once and shared (treat as read-only)."""
    c = cases()[name]
    return tuple(oracles(ev, c.shape, norm, q) for ev in c.expect)


def bound_of(o, raw=False):
    """The bound of the module docstring for the output of `o` (raw: for the grid before clipping and normalisation) and its
    parts."""
    g64, g32, m = (o['raw64'], o['raw32'], 1.0) if raw else (o['g64'], o['g32'], o['m'])
    err32 = float((g32.double() - g64).abs().max())
    T = int(o['taps'].max())
    return max(4 * err32, 2.0 ** -22 * float(g64.abs().max())) + T * 2.0 ** -30 * m, err32, T


def threshold_info(raw64, q):
    """The clipping threshold's ranks on the raw float64 grid -> (threshold's lower value, k0, k1, tied): tied = the value at rank
    k0 repeats at rank k1 > k0 (the device then never looks at the next larger value)."""
    srt = torch.sort(raw64.abs().reshape(-1)).values
    pos = np.float32(1 - q) * np.float32(srt.numel() - 1)
    k0, k1 = int(np.floor(pos)), int(np.ceil(pos))
    return float(srt[k0]), k0, k1, bool(k1 > k0 and srt[k1] == srt[k0])


def input_caps(o):
    """The two conditions on the inputs -> (entries with 0 < |raw_64| <= the raw bound, entries whose non-zero status differs
    between fp32 and fp64).  Both must be 0 for a case to be used."""
    braw, _, _ = bound_of(o, raw=True)
    r = o['raw64'].abs()
    return int(((r > 0) & (r <= braw)).sum()), int(((o['raw64'] != 0) != (o['raw32'] != 0)).sum())


def judge(out, o, label):
    """out: the device grid [C, H, W] (CPU tensor).  Prints every figure, then -> (ratio of the worst difference to the bound,
    entries that are zero in fp64 but not +-0 on the device, non-finite entries)."""
    b, err32, T = bound_of(o)
    d = float((out.double() - o['g64']).abs().max()) if out.numel() else 0.0
    nzz = int(((o['g64'] == 0) & (out != 0)).sum())
    bad = int((~torch.isfinite(out)).sum())
    ratio = d / b if b > 0 else (0.0 if d == 0 else float('inf'))
    print(f'{label}: |gpu - f64| {d:.3e}  bound {b:.3e} (err32 {err32:.3e}, max {float(o["g64"].abs().max()):.3e}, T {T}, '
          f'm {o["m"]:.4g})  ratio {ratio:.3f}  non-zero where f64 is 0: {nzz}  non-finite: {bad}', flush=True)
    return ratio, nzz, bad



# ---- the reference's fixtures ---------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BASE_FIXTURES = ('g8_voxel_meanstd', 'g8_voxel_max', 'g8_voxel_raw', 'g8_voxel_q05_meanstd', 'g8_voxel_q10_raw', 'g8_voxel_q02_max')
EDGE_FIXTURES = ('g8_voxel_e_single', 'g8_voxel_e_equal_t', 'g8_voxel_e_time', 'g8_voxel_e_sparse_q10', 'g8_voxel_e_two_int',
                 'g8_voxel_e_int_q05')


def fixture(name):
    """A g8_voxel_* fixture of the unmodified reference (oracle/gen_golden_voxel.py) -> (its arrays, (x, y, t, p) tensors, shape,
    norm_type, quantile)."""
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    norm = str(g['norm'])
    ev = tuple(torch.from_numpy(g[k]) for k in ('x', 'y', 't', 'p'))
    return g, ev, tuple(int(v) for v in g['shape']), (None if norm == 'None' else norm), float(g['quantile'])
