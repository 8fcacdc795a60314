"""The ingest edge cases of tests/ingest_cases.py on the CPU: every case reaches the edge it names, judged from the numpy oracle
alone, and `check_ordered` accepts a correct bucket layout and rejects three broken ones."""
import numpy as np
import pytest

import ingest_cases as IC

CHUNK = 1024          # csrc/ingest.hip: ING_CHUNK


def _times(c, b):
    """(t - tmin) / span of sample b in float64, as the oracle forms it."""
    t = c.samples[b][2][:c.n(b)]
    return (t - t.min()) / (t.max() - t.min())


def _bins(c, b):
    return np.clip(np.searchsorted(np.linspace(0, 1, c.nb + 1), _times(c, b)) - 1, 0, None)


def test_case_table_is_complete_and_padded():
    cs = IC.cases()
    assert tuple(cs) == IC.CASE_NAMES
    for name, c in cs.items():
        x, y, t, p, counts = c.raw()
        assert x.shape == y.shape == t.shape == p.shape == (c.B, c.N) and counts.shape == (c.B,), name
        assert t.dtype == np.int64 and p.dtype == np.float32 and counts.dtype == np.int32, name
        assert x.dtype == y.dtype == (np.int32 if c.rect_map is not None else np.float32), name
        for b in range(c.B):
            tb = t[b, :c.n(b)]
            assert (np.diff(tb) >= 0).all(), (name, b)          # voxel_input takes t[0] and t[-1] as the extrema
        ev, num_pos, xytp = IC.expected(name)
        assert ev.shape[0] == c.B and ev.shape[2] == 6 and 0 <= num_pos <= ev.shape[1], name
        assert [len(v) for v in xytp] == [c.n(b) for b in range(c.B)], name
        assert bool(np.isnan(ev).any() or any(np.isnan(v[:, 2]).any() for v in xytp)) == c.nan, name


def test_chunks_cases_reach_both_load_paths():
    cs = IC.cases()
    assert cs['chunks_2049'].N % 4 == 1 and cs['chunks_2052'].N % 4 == 0
    for name in ('chunks_2049', 'chunks_2052', 'chunks_unaligned'):
        assert tuple(cs[name].counts) == IC.CHUNK_COUNTS, name
    assert {int(n) % 4 for n in IC.CHUNK_COUNTS} == {0, 1, 3} and {(int(n) + CHUNK - 1) // CHUNK for n in IC.CHUNK_COUNTS} == {0, 1, 2, 3}
    over = cs['chunks_over']
    assert over.counts[-1] == over.N + 7 and over.n(over.B - 1) == over.N == len(over.samples[-1][0])
    ev, num_pos, xytp = IC.expected('chunks_over')
    kept = int((ev[-1, :, 5] == 1).sum())
    assert 0 < kept <= over.N and len(xytp[-1]) == over.N
    assert cs['chunks_unaligned'].unaligned and cs['chunks_unaligned'].N % 4 == 0


def test_many_chunks_needs_three_scan_passes():
    c = IC.cases()['many_chunks']
    chunks = [(c.n(b) + CHUNK - 1) // CHUNK for b in range(c.B)]
    assert chunks == [257, 513, 1] and (c.N + CHUNK - 1) // CHUNK == 513
    for b in range(2):
        x, y, _, p = c.samples[b]
        kept = (0 <= x) & (x < c.W) & (0 <= y) & (y < c.H)
        n = c.n(b)
        pad = (-n) % CHUNK
        per = lambda m: np.concatenate((m, np.zeros(pad, bool))).reshape(-1, CHUNK).sum(1)          # noqa: E731
        pos, neg = per(kept & (p == 1)), per(kept & (p == 0))
        assert len(np.unique(pos[:-1])) > 50 and len(np.unique(neg[:-1])) > 50, b
        assert len(np.unique((pos + neg)[:-1])) > 50, b          # non-constant totals per chunk
        # the carry of the second and the third pass is not the carry of the first
        assert 0 < pos[:256].sum() != pos[256:512].sum()


@pytest.mark.parametrize('nb', IC.EDGE_NB)
def test_bin_edges_land_on_and_beside_every_edge(nb):
    c = IC.cases()['bin_edges_%d' % nb]
    edges = np.linspace(0, 1, nb + 1)
    for b in range(c.B):
        t = c.samples[b][2]
        assert int(t.max() - t.min()) == IC.SPAN53 and t.min() == IC.BASE_US
        tn, bins = _times(c, b), _bins(c, b)
        assert (tn == (t - t.min()).astype(np.float64) / float(IC.SPAN53)).all()
        on = np.isin(tn, edges[1:-1])
        assert int(on.sum()) >= nb // 2
        for j in np.nonzero(on)[0]:
            i = int(np.nonzero(edges == tn[j])[0][0])
            assert bins[j] == i - 1 and bins[j + 1] == i and t[j + 1] == t[j] + 1 and t[j - 1] == t[j] - 1
        for i in range(1, nb):          # every inner edge has a stamp at most one step under it and one at most one step over it
            below, above = tn[tn <= edges[i]].max(), tn[tn > edges[i]].min()
            assert edges[i] - below <= 2.0 ** -53 and above - edges[i] <= 2.0 ** -53
        guess = np.clip(np.ceil(tn * nb) - 1, 0, None)
        if nb > 1:
            assert int((guess != bins).sum()) >= 1          # the correcting loops of bin_index are needed
        ev, _, _ = IC.expected(c.name)
        valid = ev[b][ev[b, :, 5] == 1]
        assert len(valid) == len(t) and set(valid[:, 4]) == set(range(nb))
    # both polarity blocks see every stamp
    assert (c.samples[0][3] + c.samples[1][3] == 1).all()


def test_filter_keeps_what_the_oracle_keeps():
    c = IC.cases()['filter']
    x, y, _, p = c.samples[0]
    v = IC.filter_values(c.H, c.W)
    assert np.signbit(v[0]) and v[0] == 0 and v[2] < c.W and np.nextafter(v[2], np.float32(np.inf)) == c.W and v[5] < c.H and np.isnan(v[7]) and np.isinf(v[8])
    okx = {-0.0: True, 0.0: True, float(v[2]): True, 56.0: False, 40.0: True, float(v[5]): True, float(v[6]): False, 3.5: True}
    oky = {-0.0: True, 0.0: True, float(v[2]): False, 56.0: False, 40.0: False, float(v[5]): True, float(v[6]): False, 3.5: True}
    keep = np.array([okx.get(float(a), False) and oky.get(float(b), False) for a, b in zip(x, y)])
    assert set(np.unique(x[~np.isnan(x)])) == set(np.unique(v[~np.isnan(v)])) and set(p[~np.isnan(p)]) == {0.0, 1.0, -1.0, 0.5, 2.0}
    ev, num_pos, _ = IC.expected('filter')
    pos, neg = ev[0, :num_pos], ev[0, num_pos:]
    assert num_pos == int((keep & (p == 1)).sum()) and len(neg) == int((keep & (p == 0)).sum()) and 0 < num_pos < keep.sum()
    assert np.array_equal(pos[:, :2], np.stack((y, x), -1)[keep & (p == 1)]) and np.array_equal(neg[:, :2], np.stack((y, x), -1)[keep & (p == 0)])
    assert np.signbit(ev[0, :, :2]).any() and (ev[..., 5] == 1).all()          # -0.0 passes the filter and keeps its sign


def test_padding_blocks():
    ev, num_pos, _ = IC.expected('padding')
    c = IC.cases()['padding']
    npos = (ev[:, :num_pos, 5] == 1).sum(1)
    nneg = (ev[:, num_pos:, 5] == 1).sum(1)
    assert npos[0] > 0 and nneg[0] == 0 and npos[1] == 0 and nneg[1] > 0 and npos[2] == nneg[2] == 0 and npos[3] > 0 and nneg[3] > 0
    assert num_pos == npos.max() and ev.shape[1] - num_pos == nneg.max()
    lens = [c.n(b) for b in range(c.B)]
    assert min(lens) < CHUNK < max(lens) and len({(n + CHUNK - 1) // CHUNK for n in lens}) == 2
    ev, num_pos, xytp = IC.expected('all_dropped')
    d = IC.cases()['all_dropped']
    assert ev.shape == (d.B, 0, 6) and num_pos == 0 and d.N == 1500 and [len(v) for v in xytp] == [1500, 1024, 7]


def test_degenerate_time_gives_nan_and_the_bin_past_the_last():
    c = IC.cases()['degenerate_time']
    ev, num_pos, xytp = IC.expected('degenerate_time')
    assert [c.n(b) for b in range(c.B)][:3] == [1, 5, 2]
    for b, n in ((0, 1), (1, 5)):
        rows = ev[b][ev[b, :, 5] == 1]
        assert len(rows) == n and np.isnan(rows[:, 2]).all() and (rows[:, 4] == c.nb).all() and np.isnan(xytp[b][:, 2]).all()
    rows = ev[2][ev[2, :, 5] == 1]
    assert sorted(rows[:, 2]) == [0.0, 1.0] and sorted(rows[:, 4]) == [0.0, c.nb - 1.0]
    assert not np.isnan(ev[3]).any() and (ev[:, :num_pos, 5] == 1).any(1).sum() >= 3 and (ev[:, num_pos:, 5] == 1).any(1).sum() >= 3


@pytest.mark.parametrize('name', [n for n in IC.CASE_NAMES if n.startswith('strips')])
def test_strips_sit_on_every_cell_row_border(name):
    c = IC.cases()[name]
    y = c.samples[0][1]
    for m in range(0, c.H, c.sp):
        f = np.float32(m)
        assert (y == f).any() and (y == np.nextafter(f, np.float32(np.inf))).any() and (y == np.nextafter(f, np.float32(-np.inf))).any(), m
    assert (y == c.H - 1).any()
    assert [c.n(b) for b in range(c.B)][1:] == [0, 1] and c.nb == 7 and c.ordered
    t = c.samples[0][2]
    assert set(t - IC.BASE_US) == set(IC.edge_stamps(7))
    ev, num_pos, _ = IC.expected(name)
    assert (ev[0, :num_pos, 5] == 1).sum() > 100 and (ev[0, num_pos:, 5] == 1).sum() > 100 and np.isnan(ev[2, :, 2]).sum() == 1
    # every (bin, cell row) pair is populated: whichever rows the library's strips start at, both sides of the border hold events
    rows = ev[0][ev[0, :, 5] == 1]
    pairs = set(zip(rows[:, 4].astype(int), np.floor(rows[:, 0] / np.float32(c.sp)).astype(int)))
    assert pairs == {(it, iy) for it in range(c.nb) for iy in range(c.hq)}


def test_strips_cover_a_superpixel_size_that_is_no_power_of_two():
    sps = {IC.cases()[n].sp for n in IC.CASE_NAMES if n.startswith('strips')}
    assert 3 in sps and 4 in sps
    c = IC.cases()['strips_45x63_sp3']
    assert (c.H, c.W, c.hq) == (45, 63, 15) and c.sp & (c.sp - 1)
    assert (IC.cases()['strips_48x64_sp4'].H, IC.cases()['strips_48x64_sp4'].W) == (48, 64)


def test_map_case_spills_and_leaves_the_map():
    c = IC.cases()['map']
    hs, ws = c.rect_map.shape[:2]
    m = c.rect_map
    assert (m[..., 0] < 0).any() and (m[..., 0] >= c.W).any() and (m[..., 1] < 0).any() and (m[..., 1] >= c.H).any() and np.isnan(m).any()
    assert tuple(c.counts) == IC.CHUNK_COUNTS and c.N % 4 == 0
    x, y = c.samples[-1][0], c.samples[-1][1]
    assert (x < 0).any() and (x >= ws).any() and (y < 0).any() and (y >= hs).any()
    gx, gy = c.coords(c.B - 1)
    outside = (x < 0) | (x >= ws) | (y < 0) | (y >= hs)
    assert (gx[outside] == -2).all() and (gy[outside] == -2).all() and 0 < outside.sum() < len(x)
    _, _, xytp = IC.expected('map')
    assert (xytp[-1][outside, :2] == -2).all()
    p = np.concatenate([s[3] for s in c.samples])
    assert np.isnan(p).any() and (p == 0.5).any() and (p == 2).any() and (p == -1).any()


# ---- check_ordered ----------------------------------------------------------------------------------------------------------
def _layout(ev, num_pos, nb, sp, hq, csr):
    """A bucket layout built in numpy from the oracle's tensor for strips of `csr` cell rows: each block sorted (stably) by
    key = clip(bin) * NCS + cell row // csr, the padding rows last."""
    ncs = -(-hq // csr)
    B, M = ev.shape[:2]
    out = np.zeros_like(ev)
    offs = np.zeros((B, 2, nb * ncs + 1), np.int32)
    for b in range(B):
        for pol, (s, e) in enumerate(((0, num_pos), (num_pos, M))):
            rows = ev[b, s:e]
            rows = rows[rows[:, 5] == 1]
            with np.errstate(invalid='ignore'):
                it = np.clip(rows[:, 4], 0, nb - 1).astype(int)
            iy = np.clip(np.floor(rows[:, 0] / np.float32(sp)), 0, hq - 1).astype(int)
            key = it * ncs + iy // csr
            rows = rows[np.argsort(key, kind='stable')]
            out[b, s:s + len(rows)] = rows
            offs[b, pol] = s + np.concatenate(([0], np.cumsum(np.bincount(key, minlength=nb * ncs))))
    return out, offs


@pytest.mark.parametrize('name,csr', [('strips_48x64_sp4', 5), ('strips_45x63_sp3', 4), ('strips_45x63_sp3', 15), ('degenerate_time', 3), ('padding', 10)])
def test_check_ordered_accepts_a_layout_and_rejects_three_broken_ones(name, csr):
    c = IC.cases()[name]
    ev, num_pos, _ = IC.expected(name)
    out, offs = _layout(ev, num_pos, c.nb, c.sp, c.hq, csr)
    args = (num_pos, ev, c.nb, c.sp, c.hq)
    IC.check_ordered(out, offs, *args)
    # a sample and block whose first two non-empty buckets are neighbours
    b, pol, k = next((b, pol, k) for b in range(c.B) for pol in range(2) for k in range(offs.shape[2] - 2)
                     if offs[b, pol, k + 2] > offs[b, pol, k + 1] > offs[b, pol, k])
    # 1: the last row of bucket k handed to bucket k + 1 (the rows stay where they are, the border moves)
    moved = offs.copy()
    moved[b, pol, k + 1] -= 1
    with pytest.raises(AssertionError):
        IC.check_ordered(out, moved, *args)
    # ... and the same by swapping two rows across the border
    swapped = out.copy()
    j = offs[b, pol, k + 1]
    swapped[b, [j - 1, j]] = swapped[b, [j, j - 1]]
    with pytest.raises(AssertionError):
        IC.check_ordered(swapped, offs, *args)
    # 2: one offset shifted: the table no longer starts the block where the block starts
    shifted = offs.copy()
    shifted[b, 1, 0] += 1
    with pytest.raises(AssertionError):
        IC.check_ordered(out, shifted, *args)
    # 3: one padding row that is not zero (a sentinel, a denormal, a negative zero)
    pb, ppol = next((b, pol) for b in range(c.B) for pol in range(2) if offs[b, pol, -1] < (num_pos if pol == 0 else ev.shape[1]))
    for v in (np.float32('nan'), np.float32(1e-45), np.float32(-0.0)):
        dirty = out.copy()
        dirty[pb, offs[pb, ppol, -1], 3] = v
        with pytest.raises(AssertionError):
            IC.check_ordered(dirty, offs, *args)
    # a row that is lost (replaced by a copy of its neighbour) is noticed as well
    lost = out.copy()
    lost[b, offs[b, pol, k]] = lost[b, offs[b, pol, k + 1]]
    with pytest.raises(AssertionError):
        IC.check_ordered(lost, offs, *args)
