"""Named edge cases of the DSEC event ingest (csrc/ingest.hip: count, scan, scatter, key count, ordered scatter; float and
rectification-map sources) and what each must give, from oracle/ingest_oracle.py alone.  A helper module (no fixtures, no GPU
import): tests/test_ingest_cases_host.py checks on the CPU that every case reaches the edge it names,
tests/test_gpu_ingest_cases.py runs them on the device.

Every comparison is bit for bit: the ingest is a restatement of float64 numpy arithmetic followed by one cast, so there is no
tolerance anywhere.  `check_ordered` states the bucket layout of the ordered route on its own, without the strip height the
library picks."""
import contextlib
import functools

import numpy as np

from oracle import ingest_oracle as I

BASE_US = 51_000_000_000          # a DSEC-like first stamp
SPAN53 = 1 << 53                  # a window of exactly 2^53 us: (t - tmin) / span is exact in float64
EDGE_NB = (1, 7, 15, 41, 100)
EMPTY = (np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32))


class Case:
    """samples: per sample (x, y, t_us, p) -- x, y float32 coordinates, or int32 raw indices when `rect_map` [Hs, Ws, 2] is given.
    N: row length of the padded batch; counts: what the kernel is told (None: the true lengths; a count above N is clamped to
    N by the kernels, and the oracle sees N events).  sp: the superpixel size of the loss the ordered route is run for.
    unaligned: the device test hands every input array over as a view one element into a flat buffer.  nan: the expected
    tensors hold NaN (0 / 0 times).  ordered: the case also runs on the ordered route."""

    def __init__(self, name, hw, nb, samples, N=None, counts=None, rect_map=None, sp=4, unaligned=False, nan=False, ordered=False):
        self.name, self.H, self.W, self.nb, self.samples = name, int(hw[0]), int(hw[1]), int(nb), samples
        self.N = int(N) if N is not None else max(max(len(s[0]) for s in samples), 1)
        self.counts = np.asarray(counts if counts is not None else [len(s[0]) for s in samples], dtype=np.int32)
        self.rect_map, self.sp, self.unaligned, self.nan, self.ordered = rect_map, int(sp), unaligned, nan, ordered

    @property
    def B(self):
        return len(self.samples)

    @property
    def hq(self):
        return -(-self.H // self.sp)

    def n(self, b):
        return int(min(self.counts[b], self.N))

    def raw(self):
        """-> x, y, t_us, p [B, N] and counts [B] int32.  The rows past a sample's length hold an in-image positive event with
        a stamp behind every real one: a kernel that reads them changes the counts and the time span."""
        xy = np.int32 if self.rect_map is not None else np.float32
        x = np.full((self.B, self.N), 2 if self.rect_map is not None else 0.4 * self.W, dtype=xy)
        y = np.full((self.B, self.N), 1 if self.rect_map is not None else 0.4 * self.H, dtype=xy)
        t = np.full((self.B, self.N), BASE_US + 3 * SPAN53, dtype=np.int64)
        p = np.ones((self.B, self.N), dtype=np.float32)
        for b, s in enumerate(self.samples):
            k = len(s[0])
            assert k <= self.N
            x[b, :k], y[b, :k], t[b, :k], p[b, :k] = s
        return x, y, t, p, self.counts.copy()

    def coords(self, b):
        """The float32 coordinates of sample b as the kernels see them: the arrays themselves, or rect_map[y, x] with (-2, -2)
        for an index outside the map (utils/ingest.py)."""
        x, y = self.samples[b][0], self.samples[b][1]
        if self.rect_map is None:
            return x, y
        hs, ws = self.rect_map.shape[:2]
        ok = (x >= 0) & (x < ws) & (y >= 0) & (y < hs)
        g = np.full((len(x), 2), -2.0, dtype=np.float32)
        g[ok] = self.rect_map[y[ok], x[ok]]
        return g[:, 0].copy(), g[:, 1].copy()

    def gathered(self):
        """x, y [B, N] float32 for the float route: `coords` of every sample, the padding as `raw` leaves it for that route."""
        x = np.full((self.B, self.N), 0.4 * self.W, dtype=np.float32)
        y = np.full((self.B, self.N), 0.4 * self.H, dtype=np.float32)
        for b in range(self.B):
            k = len(self.samples[b][0])
            x[b, :k], y[b, :k] = self.coords(b)
        return x, y


def _quiet(t):
    """0 / 0 only: a window whose stamps are all equal."""
    return np.errstate(invalid='ignore') if len(t) and t.max() == t.min() else contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (events [B, M, 6], num_pos, [xytp[b, :n] per sample]) from the oracle, computed once and shared (read-only)."""
    c = cases()[name]
    samples, xytp = [], []
    for b in range(c.B):
        n = c.n(b)
        if n == 0:
            samples.append(EMPTY)
            xytp.append(np.zeros((0, 4), np.float32))
            continue
        x, y = (v[:n] for v in c.coords(b))
        t, p = c.samples[b][2][:n], c.samples[b][3][:n]
        with _quiet(t):
            samples.append(I.sample_events(x, y, t, p, c.H, c.W, c.nb))
            xytp.append(I.voxel_input(x, y, t, p))
    events, num_pos = I.collate(samples)
    for a in (events, *xytp):
        a.setflags(write=False)
    return events, int(num_pos), xytp


# ---- building blocks ------------------------------------------------------------------------------------------------------
def _stamps(n, g, window_us=100_000):
    return np.sort(g.integers(0, window_us, n)).astype(np.int64) + BASE_US


def _random(n, hw, g, spill=3.0):
    """n events as the slicer delivers them: coordinates that may leave the sensor, increasing stamps, polarity in {0, 1}."""
    H, W = hw
    x = (g.random(n) * (W - 1 + 2 * spill) - spill).astype(np.float32)
    y = (g.random(n) * (H - 1 + 2 * spill) - spill).astype(np.float32)
    return x, y, _stamps(n, g), (g.random(n) > 0.45).astype(np.float32)


def edge_stamps(nb):
    """Offsets v in [0, 2^53] with v / 2^53 on, one step below and one step above every inner edge of np.linspace(0, 1, nb + 1),
    plus both ends.  An edge >= 0.5 times 2^53 is an integer, so those are hit exactly; below 0.5 the truncation lands just
    under the edge and + 1 just over it."""
    e = np.linspace(0, 1, nb + 1)
    v = {0, SPAN53}
    for i in range(1, nb):
        k = int(e[i] * SPAN53)
        v.update((k - 1, k, k + 1))
    return np.array(sorted(v), dtype=np.int64)


CHUNK_COUNTS = (0, 1, 3, 4, 5, 1023, 1024, 1025, 2049)


def _chunks(name, N, seed, counts=None, **kw):
    hw = (40, 56)
    g = np.random.default_rng(seed)
    lens = list(CHUNK_COUNTS)
    if counts is not None:
        lens[-1] = N                     # the sample that is told N + 7 holds N events
    return Case(name, hw, 15, [_random(n, hw, g) for n in lens], N=N, counts=counts, nan=True, **kw)


def case_many_chunks():
    """B = 3, 257 / 513 / 1 chunks of 1024 events: k_ingest_scan takes three passes of 256 chunks.  Polarity and the in-image
    share change from chunk to chunk, so no chunk offset is a multiple of a constant."""
    hw, lens = (40, 56), (256 * 1024 + 1, 2 * 256 * 1024 + 5, 1024)
    out = []
    for b, n in enumerate(lens):
        g = np.random.default_rng(300 + b)
        ch = np.arange(n) // 1024
        ppos = 0.1 + 0.8 * ((ch * 37 + 11 * b) % 101) / 100.0
        pin = 0.3 + 0.7 * ((ch * 53 + 7 * b) % 89) / 88.0
        inside = g.random(n) < pin
        x = np.where(inside, g.random(n) * (hw[1] - 1), hw[1] + 1 + g.random(n) * 4).astype(np.float32)
        y = (g.random(n) * (hw[0] - 1)).astype(np.float32)
        out.append((x, y, _stamps(n, g, 1_000_000), (g.random(n) < ppos).astype(np.float32)))
    return Case('many_chunks', hw, 15, out, N=2 * 256 * 1024 + 8, ordered=True)


def case_bin_edges(nb):
    """Stamps on and one step either side of every inner bin edge (edge_stamps), both polarities on every stamp across the two
    samples."""
    hw = (40, 56)
    v = edge_stamps(nb)
    g = np.random.default_rng(400 + nb)
    out = []
    for b in range(2):
        x = (g.random(len(v)) * (hw[1] - 1)).astype(np.float32)
        y = (g.random(len(v)) * (hw[0] - 1)).astype(np.float32)
        out.append((x, y, BASE_US + v, ((np.arange(len(v)) + b) % 2).astype(np.float32)))
    return Case('bin_edges_%d' % nb, hw, nb, out)


def case_degenerate_time():
    """One event (0 / 0), five events on one stamp (all 0 / 0), two events (t = 0 and 1), next to a normal sample."""
    hw = (40, 56)
    g = np.random.default_rng(500)
    f = lambda *v: np.array(v, dtype=np.float32)          # noqa: E731
    one = (f(10.5), f(7.25), np.array([BASE_US + 17], np.int64), f(1))
    same = (f(1.5, 20.25, 30.0, 55.5, 8.0), f(3.0, 39.5, 12.25, 0.5, 20.0), np.full(5, BASE_US + 99, np.int64), f(1, 0, 0, 1, 0))
    two = (f(2.0, 50.0), f(30.0, 4.0), np.array([BASE_US, BASE_US + 1], np.int64), f(0, 1))
    return Case('degenerate_time', hw, 5, [one, same, two, _random(300, hw, g, spill=1.0)], nan=True, ordered=True)


FILTER_P = (0.0, 1.0, -1.0, 0.5, 2.0, float('nan'))


def filter_values(H, W):
    w, h = np.float32(W), np.float32(H)
    return np.array([-0.0, 0.0, np.nextafter(w, np.float32(0)), w, h, np.nextafter(h, np.float32(0)), -1e-7, float('nan'), float('inf'), 3.5],
                    dtype=np.float32)


def case_filter():
    """Every pair of the coordinate values of `filter_values` in (x, y), under every polarity of FILTER_P."""
    hw = (40, 56)
    v = filter_values(*hw)
    xs, ys, ps = np.meshgrid(v, v, np.array(FILTER_P, np.float32), indexing='ij')
    n = xs.size
    return Case('filter', hw, 5, [(xs.reshape(-1).copy(), ys.reshape(-1).copy(), BASE_US + 13 * np.arange(n, dtype=np.int64), ps.reshape(-1).copy())])


def case_padding():
    """B = 4, lengths either side of a chunk: positives only, negatives only, everything outside the image, mixed."""
    hw = (40, 56)
    g = np.random.default_rng(600)
    pos = _random(1023, hw, g)
    neg = _random(1025, hw, g)
    out = _random(1500, hw, g)
    mixed = _random(1030, hw, g)
    pos[3][:] = 1
    neg[3][:] = 0
    out[0][::2] += hw[1] + 4
    out[1][1::2] -= hw[0] + 4
    return Case('padding', hw, 15, [pos, neg, out, mixed], ordered=True)


def case_all_dropped():
    """Every event of every sample is dropped (outside the image, or a polarity that is neither 0 nor 1): M == 0 while N = 1500."""
    hw = (40, 56)
    g = np.random.default_rng(610)
    out = []
    for b, n in enumerate((1500, 1024, 7)):
        x, y, t, p = _random(n, hw, g)
        if b == 1:
            p[:] = 0.5
        else:
            x += hw[1] + 4
        out.append((x, y, t, p))
    return Case('all_dropped', hw, 15, out, N=1500, ordered=True)


def strip_rows(H, sp):
    """y on every multiple of sp inside the image, one float step either side, and the last image row."""
    m = np.arange(0, H, sp, dtype=np.float32)
    lo, hi = np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf))
    return np.unique(np.concatenate((m, lo, hi, [np.float32(H - 1), np.nextafter(np.float32(H), np.float32(0))])).astype(np.float32))


def case_strips(name, hw, sp):
    """Ordered route: every y of `strip_rows` under every stamp of edge_stamps(7); a normal, an empty and a one-event sample."""
    ys, v = strip_rows(hw[0], sp), edge_stamps(7)
    g = np.random.default_rng(700 + sp + hw[1])
    iy, it = np.meshgrid(np.arange(len(ys)), np.arange(len(v)), indexing='ij')
    iy, it = iy.T.reshape(-1), it.T.reshape(-1)                      # stamps non-decreasing
    x = (g.random(iy.size) * (hw[1] - 1)).astype(np.float32)
    normal = (x, ys[iy].copy(), BASE_US + v[it], ((iy + it) % 2).astype(np.float32))
    none = tuple(np.zeros(0, d) for d in (np.float32, np.float32, np.int64, np.float32))
    f = lambda *a: np.array(a, dtype=np.float32)          # noqa: E731
    one = (f(5.0), f(2.0 * sp), np.array([BASE_US + 5], np.int64), f(0))
    return Case(name, hw, 7, [normal, none, one], sp=sp, nan=True, ordered=True)


def case_map():
    """The chunk lengths with int32 indices into a [30, 44, 2] map whose values spill outside the 40 x 56 image (the filter's
    coordinate values among them), indices outside the map, and the polarities of FILTER_P."""
    hw, hs, ws = (40, 56), 30, 44
    g = np.random.default_rng(800)
    m = np.stack((g.random((hs, ws)) * (hw[1] + 6) - 3, g.random((hs, ws)) * (hw[0] + 6) - 3), -1).astype(np.float32)
    v = filter_values(*hw)
    m[0, :len(v), 0] = v
    m[1, :len(v), 1] = v
    pv = np.array(FILTER_P + (0.0, 1.0, 0.0, 1.0, 0.0, 1.0), np.float32)
    out = []
    for n in CHUNK_COUNTS:
        x = g.integers(-2, ws + 2, n).astype(np.int32)
        y = g.integers(-2, hs + 2, n).astype(np.int32)
        y[::5] = g.integers(0, 2, len(y[::5]))                       # the rows of the map that hold the filter's values
        out.append((x, y, _stamps(n, g), pv[g.integers(0, len(pv), n)]))
    return Case('map', hw, 15, out, N=2052, rect_map=m, nan=True, ordered=True)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [_chunks('chunks_2049', 2049, 201), _chunks('chunks_2052', 2052, 202),
          _chunks('chunks_over', 2052, 203, counts=CHUNK_COUNTS[:-1] + (2052 + 7,)),
          _chunks('chunks_unaligned', 2052, 204, unaligned=True),
          case_many_chunks(), *(case_bin_edges(nb) for nb in EDGE_NB), case_degenerate_time(), case_filter(), case_padding(),
          case_all_dropped(), case_strips('strips_48x64_sp4', (48, 64), 4), case_strips('strips_45x63_sp3', (45, 63), 3),
          case_strips('strips_160x640_sp4', (160, 640), 4), case_map()]
    return {c.name: c for c in cs}


CASE_NAMES = ('chunks_2049', 'chunks_2052', 'chunks_over', 'chunks_unaligned', 'many_chunks', 'bin_edges_1', 'bin_edges_7',
              'bin_edges_15', 'bin_edges_41', 'bin_edges_100', 'degenerate_time', 'filter', 'padding', 'all_dropped',
              'strips_48x64_sp4', 'strips_45x63_sp3', 'strips_160x640_sp4', 'map')
RAW_ABI_CASES = ('chunks_2049', 'chunks_2052', 'chunks_over', 'chunks_unaligned', 'padding', 'all_dropped', 'many_chunks', 'degenerate_time')
ORDERED_CASES = tuple(n for n in CASE_NAMES if n.startswith('strips') or n in ('degenerate_time', 'padding', 'all_dropped', 'many_chunks', 'map'))
# 160 x 640 at superpixel 4 is the smallest of the strips images on which the library splits the LUT rows into more than one
# strip (its strips hold 48 KB of 16-byte cells: 19 rows of 160 cells); on the two small images every bin is one bucket.
MULTI_STRIP_CASES = ('strips_160x640_sp4',)


# ---- the ordered layout, stated on its own --------------------------------------------------------------------------------
def row_bits(rows):
    """Rows as sortable uint32 bit patterns, every NaN as one pattern (-0.0 and 0.0 stay apart) -> [n, 6] sorted by row."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    bits = r.view(np.uint32).copy()
    bits[np.isnan(r)] = 0x7FC00000
    return bits[np.lexsort(bits.T[::-1])] if len(bits) else bits


def check_ordered(events, offsets, num_pos, unordered_events, nb, sp, hq):
    """The bucket layout of `ingest_events(order_for=)` / `FocusLoss.order_events`: events [B, M, 6] and offsets [B, 2, nb * NCS + 1]
    (numpy) against the time-ordered tensor `unordered_events` of the oracle.  Raises AssertionError on the first violation."""
    events, offsets, ref = np.asarray(events), np.asarray(offsets), np.asarray(unordered_events)
    B, M = events.shape[:2]
    assert ref.shape == events.shape and offsets.shape[:2] == (B, 2) and (offsets.shape[2] - 1) % nb == 0, (events.shape, ref.shape, offsets.shape)
    ncs = (offsets.shape[2] - 1) // nb
    assert ncs >= 1
    for b in range(B):
        for pol in range(2):
            o = offsets[b, pol].astype(np.int64)
            start, end = (0, num_pos) if pol == 0 else (num_pos, M)
            assert (np.diff(o) >= 0).all() and o[0] == start and o[-1] <= end, (b, pol, 'offsets')
            assert not events[b, o[-1]:end].view(np.uint32).any(), (b, pol, 'padding rows are not zero')
            want = ref[b, start:end]
            want = want[want[:, 5] == 1]
            assert np.array_equal(row_bits(events[b, start:o[-1]]), row_bits(want)), (b, pol, 'rows differ from the oracle block')
            for it in range(nb):
                last = -1
                for s in range(ncs):
                    k = it * ncs + s
                    rows = events[b, o[k]:o[k + 1]]
                    if not len(rows):
                        continue
                    with np.errstate(invalid='ignore'):
                        bins = np.clip(rows[:, 4], 0, nb - 1)
                    assert (bins == it).all() and (rows[:, 5] == 1).all(), (b, pol, k, 'bin')
                    iy = np.clip(np.floor(rows[:, 0].astype(np.float32) / np.float32(sp)), 0, hq - 1)
                    assert iy.min() > last, (b, pol, k, 'strips overlap or decrease')
                    last = iy.max()
