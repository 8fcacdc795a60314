"""utils.ingest_raw_events (csrc/ingest.hip, the window kernels) against the fixtures of the unmodified reference
(tests/golden/g14_window_*.npz) and the numpy restatement tests/ingest_window_oracle.py -- bit for bit, no tolerances."""
import numpy as np
import pytest
import torch

import ingest_window_oracle as W

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
XY = {'int32': torch.int32, 'fp32': torch.float32}
P = {'int64': torch.int64, 'fp32': torch.float32}


def _run(dataset, x, y, t, p, counts, nb, xy='int32', pt='int64', **kw):
    from motionpriorcmax_amd.utils import ingest_raw_events
    dev = torch.device(DEV)
    out = ingest_raw_events(torch.from_numpy(x).to(dev, XY[xy]), torch.from_numpy(y).to(dev, XY[xy]), torch.from_numpy(t).to(dev),
                            torch.from_numpy(p).to(dev, P[pt]), torch.from_numpy(np.asarray(counts, np.int32)), nb, dataset, **kw)
    assert out['events'].dtype == torch.float32 and out['events'].is_contiguous()
    return out['events'].cpu().numpy(), out['num_pos_events']


# ---- the reference's own output ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,split', [('g14_window_evimo2_split', True), ('g14_window_evimo2_single', False)])
@pytest.mark.parametrize('xy,pt', [('int32', 'int64'), ('fp32', 'fp32')])
def test_evimo2_fixture(name, split, xy, pt):
    g = W.load_window(name)
    ev, num_pos = _run('evimo2', g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']), xy, pt,
                       flow_duration_ms=int(g['flow_duration_ms']), polarity_aware_batching=split)
    assert num_pos == int(g['num_pos_events'])
    np.testing.assert_array_equal(ev, g['events'])


@pytest.mark.parametrize('split', [True, False])
def test_multiflow_fixture(split):
    g = W.load_window('g14_window_multiflow')
    ev, num_pos = _run('multiflow', g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']), polarity_aware_batching=split)
    assert num_pos == int(g['num_pos_events' if split else 'num_pos_events_single'])
    np.testing.assert_array_equal(ev, g['events' if split else 'events_single'])


def test_evimo2_fixture_xy_scale():
    """X_SCALE / Y_SCALE (unpinned): one fp32 multiply per coordinate as the row is written; padding rows stay zero."""
    g = W.load_window('g14_window_evimo2_split')
    ev, _ = _run('evimo2', g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']),
                 flow_duration_ms=int(g['flow_duration_ms']), xy_scale=(0.8, 0.8))
    want = torch.from_numpy(g['events']).clone()
    want[..., 0] = want[..., 0] * 0.8          # torch fp32: the scalar is rounded to fp32, one multiply
    want[..., 1] = want[..., 1] * 0.8
    np.testing.assert_array_equal(ev, want.numpy())
    pad = ev[..., 5] == 0
    assert pad.any() and not ev[pad].any()
    # the two scales are not swapped: column 0 is y
    ev2, _ = _run('evimo2', g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']),
                  flow_duration_ms=int(g['flow_duration_ms']), xy_scale=(0.5, 0.25))
    np.testing.assert_array_equal(ev2[..., 0], g['events'][..., 0] * np.float32(0.25))
    np.testing.assert_array_equal(ev2[..., 1], g['events'][..., 1] * np.float32(0.5))


# ---- edge cases against the restatement -------------------------------------------------------------------------------------
COUNTS = [0, 1, 1023, 1024, 1025, 4097]          # around the 1024-event chunk of the kernels; an empty and a one-event sample


def _ragged(N, seed, span_us=700_000, t0=100_000_000):
    """[len(COUNTS), N] windows of COUNTS events spread over `span_us`, stamps from 100 s on, coordinates of a 480 x 640 sensor."""
    g = np.random.default_rng(seed)
    B = len(COUNTS)
    x = np.zeros((B, N), np.int32); y = np.zeros((B, N), np.int32); t = np.zeros((B, N), np.int64); p = np.zeros((B, N), np.int64)
    for b, n in enumerate(COUNTS):
        x[b, :n] = g.integers(0, 640, n); y[b, :n] = g.integers(0, 480, n)
        t[b, :n] = t0 + 1000 * b + np.sort(g.integers(0, span_us, n))
        p[b, :n] = g.random(n) > 0.4
    return x, y, t, p


@pytest.mark.parametrize('N', [4097, 4100])          # element-wise loads / 16-byte loads (N a multiple of 4)
@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('dataset', ['evimo2', 'multiflow'])
def test_ragged_counts_around_the_chunk(dataset, split, N):
    x, y, t, p = _ragged(N, seed=5)
    kw = dict(flow_duration_ms=300) if dataset == 'evimo2' else {}
    want, num_pos = W.restate(dataset, x, y, t, p, COUNTS, 41, polarity_aware_batching=split, **kw)
    if dataset == 'evimo2':          # the cut is inside the window and inside a later chunk than the first for the long sample
        kept = (want[..., 5] == 1).sum(1)
        assert kept[0] == 0 and kept[1] == 1 and 1024 < COUNTS[5] - kept[5] < COUNTS[5] - 1024
    for xy, pt in (('int32', 'int64'), ('fp32', 'fp32'), ('int32', 'fp32')):
        ev, got_pos = _run(dataset, x, y, t, p, COUNTS, 41, xy, pt, polarity_aware_batching=split, **kw)
        assert got_pos == num_pos
        np.testing.assert_array_equal(ev, want)          # (NaN == NaN here: the one-event MultiFlow window divides 0 by 0)


def test_evimo2_window_shorter_than_the_duration_keeps_everything():
    x, y, t, p = _ragged(4100, seed=6, span_us=100_000)
    want, num_pos = W.restate('evimo2', x, y, t, p, COUNTS, 41, flow_duration_ms=300)
    assert ((want[..., 5] == 1).sum(1) == np.array(COUNTS)).all()
    ev, got_pos = _run('evimo2', x, y, t, p, COUNTS, 41, flow_duration_ms=300)
    assert got_pos == num_pos
    np.testing.assert_array_equal(ev, want)


def test_evimo2_stamps_that_round_onto_ts_start_are_dropped():
    """ts_start = fp32(100 300 000) - 300 000 = 100 000 000 exactly; one fp32 ulp is 8 us there, so the int64 stamps
    100 000 001 .. 100 000 004 are 100 000 000 in fp32: not greater than ts_start, dropped -- an int64 or float64 cut keeps them."""
    t = np.array([[99_999_000, 100_000_000, 100_000_001, 100_000_002, 100_000_003, 100_000_004, 100_000_005, 100_100_000, 100_300_000]],
                 np.int64)
    n = t.shape[1]
    x = np.arange(n, dtype=np.int32)[None]; y = x + 10; p = (np.arange(n) % 2).astype(np.int64)[None]
    want, _ = W.restate('evimo2', x, y, t, p, [n], 41, flow_duration_ms=300, polarity_aware_batching=False)
    assert want.shape[1] == 3 and (want[0, :, 1] == [6, 7, 8]).all()          # (x = the event's index)
    for split in (False, True):
        want, num_pos = W.restate('evimo2', x, y, t, p, [n], 41, flow_duration_ms=300, polarity_aware_batching=split)
        ev, got_pos = _run('evimo2', x, y, t, p, [n], 41, flow_duration_ms=300, polarity_aware_batching=split)
        assert got_pos == num_pos
        np.testing.assert_array_equal(ev, want)


def test_evimo2_time_on_a_bin_edge_falls_into_the_lower_bin():
    """num_bins = 4, last stamp 400 000, 400 ms: ts_start = 0, t = 0.25 and 0.5 exactly -- searchsorted(side='left') - 1."""
    t = np.array([[50_000, 100_000, 200_000, 300_000, 400_000]], np.int64)
    x = np.arange(5, dtype=np.int32)[None]; p = np.ones((1, 5), np.int64)
    ev, _ = _run('evimo2', x, x, t, p, [5], 4, flow_duration_ms=400, polarity_aware_batching=False)
    want, _ = W.restate('evimo2', x, x, t, p, [5], 4, flow_duration_ms=400, polarity_aware_batching=False)
    np.testing.assert_array_equal(ev, want)
    np.testing.assert_array_equal(ev[0, :, 2], np.array([0.125, 0.25, 0.5, 0.75, 1.0], np.float32))
    np.testing.assert_array_equal(ev[0, :, 4], np.array([0, 0, 1, 2, 3], np.float32))


def test_empty_batch_and_other_dtypes():
    """counts all zero -> [B, 0, 6]; int16 coordinates / uint8 polarity are converted with torch first."""
    from motionpriorcmax_amd.utils import ingest_raw_events
    g = W.load_window('g14_window_evimo2_split')
    dev = torch.device(DEV)
    a = [torch.from_numpy(g[k]).to(dev) for k in ('x', 'y', 't_us', 'p')]
    out = ingest_raw_events(*a, torch.zeros(3, dtype=torch.int32), 41, 'evimo2', flow_duration_ms=300)
    assert out['events'].shape == (3, 0, 6) and out['num_pos_events'] == 0
    out = ingest_raw_events(a[0].to(torch.int16), a[1].to(torch.int16), a[2], a[3].to(torch.uint8), torch.from_numpy(g['counts']), 41,
                            'evimo2', flow_duration_ms=300)
    np.testing.assert_array_equal(out['events'].cpu().numpy(), g['events'])


# ---- downstream ----------------------------------------------------------------------------------------------------------------
def test_result_feeds_the_loss_and_order_for_is_bit_identical():
    """EVIMO2 settings (41 bins, smoothness on flow_to_next) on a 48 x 64 image, coordinates scaled from a 60 x 80 sensor by 0.8."""
    from motionpriorcmax_amd import LossFactory
    from motionpriorcmax_amd.utils import ingest_raw_events
    from oracle import focus_oracle as O
    H, Wd, nb = 48, 64, 41
    g = np.random.default_rng(8)
    ns = [6000, 4500]
    N = max(ns)
    x = np.zeros((2, N), np.int32); y = np.zeros((2, N), np.int32); t = np.zeros((2, N), np.int64); p = np.zeros((2, N), np.int64)
    for b, n in enumerate(ns):
        x[b, :n] = g.integers(0, 80, n); y[b, :n] = g.integers(0, 60, n)
        t[b, :n] = 100_000_000 + np.sort(g.integers(0, 700_000, n)); p[b, :n] = g.random(n) > 0.5
    cfg = dict(image_shape=(H, Wd), num_tref=1, num_bins=nb, num_knn=32, smooth_weight=0.06, lut_superpixel_size=4,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_next')
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    dev = torch.device(DEV)
    a = [torch.from_numpy(v).to(dev) for v in (x, y, t, p)]
    cnt = torch.tensor(ns, dtype=torch.int32)
    kw = dict(flow_duration_ms=300, xy_scale=(0.8, 0.8))
    plain = ingest_raw_events(*a, cnt, nb, 'evimo2', **kw)
    ordered = ingest_raw_events(*a, cnt, nb, 'evimo2', order_for=L, **kw)
    assert 'event_offsets' in ordered and ordered['num_pos_events'] == plain['num_pos_events']
    assert float(plain['events'][..., 0].max()) < H and float(plain['events'][..., 1].max()) < Wd
    gen = torch.Generator().manual_seed(1)
    times = torch.cat((torch.tensor([0.41]), O.bin_mid_times(nb)))
    traj = O.trajectories_at(torch.randn(2, 1, 2, H, Wd, generator=gen), times, O.tile_mask((H, Wd), 4), 1, 'polynomial')
    res = []
    for batch in (plain, ordered):
        tg = traj.to(dev).requires_grad_(True)
        loss, _, misc = L.calc(tg, times.to(dev), batch)
        loss.backward()
        res.append((loss.detach(), tg.grad, misc['iwes']))
    assert torch.isfinite(res[0][0]).item() and torch.isfinite(res[0][1]).all() and float(res[0][1].abs().sum()) > 0
    assert all(torch.equal(u, v) for u, v in zip(*res))
