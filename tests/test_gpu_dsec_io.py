"""The DSEC sample on the device: rectification inside the ingest kernels (csrc/ingest.hip, `ingest_events(rectify_map=)`), the
ground-truth targets and the flow error straight from the 16-bit payload, and the benchmark export (csrc/dsec_io.hip).
Cases and restatements: tests/dsec_io_cases.py; fixtures of the unmodified reference: tests/golden/g20_dsec_*.npz."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import dsec_io_cases as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u16(t):
    """a uint16 tensor as a numpy array (through its bit pattern)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@contextlib.contextmanager
def _no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode('default')


# ---- A: ingest with a rectification map --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _window(hs=K.H, ws=K.W):
    m = K.rectify_map(hs, ws)
    x, y, t, p, counts = K.raw_window(hs, ws)
    d = dict(m=m, x=x, y=y, t=t, p=p, counts=counts)
    d['dev'] = {k: _dev(v) for k, v in d.items() if k != 'counts'}
    return d


@functools.lru_cache(maxsize=None)
def _loss():
    from motionpriorcmax_amd import LossFactory
    cfg = dict(image_shape=(K.H, K.W), num_tref=1, num_bins=K.NB, num_knn=32, smooth_weight=0.003, lut_superpixel_size=4,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _with_map(w, x=None, y=None, **kw):
    from motionpriorcmax_amd.utils import ingest_events
    g = w['dev']
    return ingest_events(g['x'] if x is None else x, g['y'] if y is None else y, g['t'], g['p'], torch.from_numpy(w['counts']),
                         (K.H, K.W), K.NB, rectify_map=g['m'], **kw)


def _gathered(w, x=None, y=None):
    """rectify_ev_map[y, x] by torch on the device: what a caller of the float path has to run first."""
    g = w['dev']
    r = g['m'][(g['y'] if y is None else y).long(), (g['x'] if x is None else x).long()]
    return r[..., 0].contiguous(), r[..., 1].contiguous()


def _float_path(w, xr, yr, **kw):
    from motionpriorcmax_amd.utils import ingest_events
    g = w['dev']
    return ingest_events(xr, yr, g['t'], g['p'], torch.from_numpy(w['counts']), (K.H, K.W), K.NB, **kw)


def _assert_same(got, ref, ordered):
    assert got['num_pos_events'] == ref['num_pos_events']
    assert (got['xytp'] is None) == (ref['xytp'] is None)
    if got['xytp'] is not None:
        a, b = got['xytp'].view(torch.int32), ref['xytp'].view(torch.int32)          # bit patterns: NaN entries and -0.0 count
        w = torch.arange(a.shape[1], device=a.device)[None, :, None] < torch.as_tensor(_window()['counts'], device=a.device)[:, None, None]
        assert torch.equal(a * w, b * w)          # (rows beyond counts[b] are not written by either path)
    if not ordered:
        assert torch.equal(got['events'], ref['events'])
        return
    # bucket order: the kernel's contract leaves the order INSIDE a (time bin, LUT strip) bucket open (LDS atomics hand out the
    # rows), so two runs of one kernel may differ there.  The table must be equal, and bucket by bucket the rows, exactly.
    assert ('event_offsets' in got) == ('event_offsets' in ref)
    assert torch.equal(got['event_offsets'], ref['event_offsets'])
    offs = got['event_offsets'].cpu().numpy()
    ea, eb = got['events'].cpu().numpy(), ref['events'].cpu().numpy()
    assert ea.shape == eb.shape
    num_pos, M = got['num_pos_events'], ea.shape[1]
    for b in range(ea.shape[0]):
        for pol in range(2):
            o = offs[b, pol]
            end = num_pos if pol == 0 else M
            assert not ea[b, o[-1]:end].any() and not eb[b, o[-1]:end].any()
            for k in np.nonzero(np.diff(o))[0]:
                ra, rb = ea[b, o[k]:o[k + 1]], eb[b, o[k]:o[k + 1]]
                assert np.array_equal(ra[np.lexsort(ra.T[::-1])], rb[np.lexsort(rb.T[::-1])]), (b, pol, k)


@pytest.mark.parametrize('voxel', [False, True])
@pytest.mark.parametrize('ordered', [False, True])
def test_ingest_with_map_equals_float_path_on_gathered_coordinates(voxel, ordered):
    """A gather is exact: `events`, `num_pos_events`, `xytp` (and `event_offsets`) equal those of the float entry points fed
    m[y, x, 0], m[y, x, 1]; count, scatter, key count and ordered scatter all go through the map source."""
    w = _window()
    kw = dict(want_voxel_input=voxel, order_for=_loss() if ordered else None)
    got = _with_map(w, **kw)
    ref = _float_path(w, *_gathered(w), **kw)
    if ordered:
        assert 'event_offsets' in got          # this shape has a bucketed layout: the ordered kernels ran
    _assert_same(got, ref, ordered)


def test_ingest_with_map_equals_oracle_and_reference_fixture():
    w = _window()
    got = _with_map(w)
    ev, num_pos = K.reference_events(w['m'], w['x'], w['y'], w['t'], w['p'], w['counts'], K.H, K.W, K.NB)
    assert got['num_pos_events'] == num_pos
    assert np.array_equal(got['events'].cpu().numpy(), ev)
    g = K.load('g20_dsec_sample')
    assert got['num_pos_events'] == int(g['num_pos_events'])
    assert np.array_equal(got['events'].cpu().numpy(), g['events'])
    assert 0 < int((ev[..., 5] == 1).sum()) < int(w['counts'].sum())          # rows were dropped, rows were kept


def test_voxel_grid_from_rectified_xytp():
    from motionpriorcmax_amd.utils import voxel_grids
    w = _window()
    cnt = torch.from_numpy(w['counts'])
    got = voxel_grids(_with_map(w, want_voxel_input=True)['xytp'], cnt, (K.NB, K.H, K.W), 'mean_std')
    ref = voxel_grids(_float_path(w, *_gathered(w), want_voxel_input=True)['xytp'], cnt, (K.NB, K.H, K.W), 'mean_std')
    assert torch.isfinite(got).all() and bool((got != 0).any())
    assert torch.equal(got, ref)


@pytest.mark.parametrize('dtype', [torch.int16, torch.uint16, torch.int64])
def test_index_dtypes(dtype):
    w = _window()
    ref = _with_map(w, want_voxel_input=True)
    conv = (lambda a: _dev(a.astype(np.uint16))) if dtype == torch.uint16 else (lambda a: _dev(a).to(dtype))
    got = _with_map(w, x=conv(w['x']), y=conv(w['y']), want_voxel_input=True)
    _assert_same(got, ref, False)


def test_float_indices_raise():
    w = _window()
    with pytest.raises(TypeError):
        _with_map(w, x=w['dev']['x'].float())
    with pytest.raises(TypeError):
        _with_map(w, y=w['dev']['y'].double())


def test_indices_outside_the_map_are_dropped():
    """UNPINNED in the reference (it raises or wraps): x >= Ws, y >= Hs and negative indices are absent from `events` and carry
    (-2, -2) in `xytp`; every other row is what it was."""
    w = _window()
    x, y = w['x'].copy(), w['y'].copy()
    bad = {0: [(100, K.W, 3), (101, 5, K.H), (1500, -1, 7), (1501, 9, -1), (4097, 70000, 2), (2000, -2**31, -2**31), (2001, K.W - 1, K.H)],
           1: [(500, K.W, K.H)], 2: [(255, -1, -1), (129, 2**31 - 1, 0)]}
    rows = {b: [r for r, _, _ in v] for b, v in bad.items()}
    for b, v in bad.items():
        for r, xv, yv in v:
            assert 0 < r < w['counts'][b] - 1          # (not the first or last event: the time extrema stay)
            x[b, r], y[b, r] = xv, yv
    got = _with_map(w, x=_dev(x), y=_dev(y), want_voxel_input=True)
    # the same window without those rows, by the restatement
    keep = [np.setdiff1d(np.arange(c), rows[b]) for b, c in enumerate(w['counts'])]
    samples = []
    from oracle import ingest_oracle as I
    for b, c in enumerate(w['counts']):
        xr, yr = K.gather(w['m'], w['x'][b, :c], w['y'][b, :c])
        t = (w['t'][b, :c] - w['t'][b, :c].min()) / (w['t'][b, :c].max() - w['t'][b, :c].min())
        with np.errstate(invalid='ignore'):
            pos, neg = I.sample_events(xr, yr, w['t'][b, :c], w['p'][b, :c], K.H, K.W, K.NB)
        # sample_events on the full window, then the rows of the bad events taken out again (they keep their time and bin)
        full = np.column_stack((yr, xr, t, w['p'][b, :c])).astype(np.float32)
        def without(block):
            drop = {tuple(full[r]) for r in rows[b]}
            return np.array([e for e in block if tuple(e[:4]) not in drop], np.float32).reshape(-1, 5)
        samples.append((without(pos), without(neg)))
    ev, num_pos = I.collate(samples)
    assert got['num_pos_events'] == num_pos and np.array_equal(got['events'].cpu().numpy(), ev)
    clean = _with_map(w, want_voxel_input=True)['xytp'].cpu().numpy()
    xytp = got['xytp'].cpu().numpy()
    for b, c in enumerate(w['counts']):
        assert (xytp[b, rows[b], :2] == -2.0).all()
        assert np.array_equal(xytp[b, rows[b], 2:], clean[b, rows[b], 2:])
        assert np.array_equal(xytp[b, keep[b]], clean[b, keep[b]], equal_nan=True)


def test_map_of_another_size_than_the_image():
    """Sensor 40 x 70 against an image of 48 x 64."""
    w = _window(40, 70)
    got = _with_map(w, want_voxel_input=True)
    assert np.array_equal(got['xytp'][0, :, 0].cpu().numpy(), K.gather(w['m'], w['x'][0], w['y'][0])[0], equal_nan=True)
    ref = _float_path(w, *_gathered(w), want_voxel_input=True)
    assert torch.equal(got['events'], ref['events']) and got['num_pos_events'] == ref['num_pos_events']
    ev, num_pos = K.reference_events(w['m'], w['x'], w['y'], w['t'], w['p'], w['counts'], K.H, K.W, K.NB)
    assert got['num_pos_events'] == num_pos and np.array_equal(got['events'].cpu().numpy(), ev)
    assert (ev[..., 1] >= 60).any() and ev[..., 0].max() < 44          # x reaches the image's right edge; y never the lower one


def test_map_arguments_are_checked():
    w = _window()
    from motionpriorcmax_amd.utils import ingest_events
    g = w['dev']
    args = (g['x'], g['y'], g['t'], g['p'], torch.from_numpy(w['counts']), (K.H, K.W), K.NB)
    with pytest.raises(ValueError):
        ingest_events(*args, rectify_map=g['m'][..., 0])
    with pytest.raises(ValueError):
        ingest_events(*args, rectify_map=g['m'].double())
    with pytest.raises(ValueError):
        ingest_events(*args, rectify_map=g['m'].permute(1, 0, 2))
    with pytest.raises(RuntimeError):
        ingest_events(*args, rectify_map=g['m'].cpu())


# ---- B: targets and error from the payload -----------------------------------------------------------------------------
SHAPES_B = [(48, 64), (5, 7)]          # 5 x 7: H * W no multiple of 4, the one-pixel-per-thread path


@pytest.mark.parametrize('hw', SHAPES_B)
def test_targets_equal_restatement(hw):
    from motionpriorcmax_amd.utils import dsec_flow_targets
    png = K.payload(2, *hw)
    flow, valid = K.decode(png)
    d = _dev(png)
    with _no_sync():
        out = dsec_flow_targets(d)
        one = dsec_flow_targets(d[1])
    assert out['forward_flow'].dtype == torch.float32 and out['flow_valid'].dtype == torch.bool
    assert out['forward_flow'].shape == (2, 2) + hw and out['flow_valid'].shape == (2,) + hw
    assert np.array_equal(out['forward_flow'].cpu().numpy(), flow) and np.array_equal(out['flow_valid'].cpu().numpy(), valid)
    assert np.array_equal(one['forward_flow'].cpu().numpy(), flow[1]) and np.array_equal(one['flow_valid'].cpu().numpy(), valid[1])
    for other in (d.view(torch.int16), _dev(png.astype(np.int32))):
        o = dsec_flow_targets(other)
        assert torch.equal(o['forward_flow'], out['forward_flow']) and torch.equal(o['flow_valid'], out['flow_valid'])
    with pytest.raises(TypeError):
        dsec_flow_targets(d.view(torch.int16).float())


def test_targets_equal_reference_fixture():
    from motionpriorcmax_amd.utils import dsec_flow_targets
    g = K.load('g20_dsec_sample')
    out = dsec_flow_targets(_dev(g['png16']))
    assert np.array_equal(out['forward_flow'].cpu().numpy(), g['forward_flow'])
    assert np.array_equal(out['flow_valid'].cpu().numpy(), g['flow_valid'])


@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('hw', SHAPES_B)
def test_error_from_payload(hw, with_scale):
    """Against the float64 restatement of flow.py:18-70 by the bound tests/test_gpu_flow.py holds calculate_flow_error to, and
    against calculate_flow_error on the decoded targets: the per-pixel body is shared and the pixels of a thread and the order of
    the sums are the same, hence the same bits.  Sample 1 of the second variant has no valid pixel (n_points = 1e-5)."""
    from motionpriorcmax_amd.utils import calculate_flow_error, dsec_flow_error, dsec_flow_targets, OpticalFlowError
    for empty in (False, True):
        png = K.payload(2, *hw)
        if empty:
            png[1, ..., 2] = 0
        gt, valid = K.decode(png)
        pr = K.prediction(gt)
        ts = np.array([[0.7], [1.3]], np.float32) if with_scale else None
        ref = K.flow_error64(gt, pr, valid, ts)
        d, dp, dts = _dev(png), _dev(pr), None if ts is None else _dev(ts)
        with _no_sync():
            got = dsec_flow_error(d, dp, dts)
        tg = dsec_flow_targets(d)
        two = calculate_flow_error(tg['forward_flow'], dp, tg['flow_valid'], dts)
        for k in K.FE_KEYS:
            print(hw, with_scale, empty, k, float(got[k]), ref[k], abs(float(got[k]) - ref[k]) / abs(ref[k]))
        for k in K.FE_KEYS:
            assert ref[k] > 0
            assert abs(float(got[k]) - ref[k]) <= K.FE_RTOL * abs(ref[k]), k
            assert abs(float(got[k]) - float(two[k])) <= K.FE_RTOL * abs(ref[k]), k
            assert torch.equal(got[k], two[k]), k
        if ts is None:
            run = OpticalFlowError.run({'flow': dp}, {'flow_png16': d})
            old = OpticalFlowError.run({'flow': dp}, {'forward_flow': tg['forward_flow'], 'flow_valid': tg['flow_valid'], 'flow_png16': d})
            assert all(torch.equal(run[k], got[k]) and torch.equal(old[k], two[k]) for k in K.FE_KEYS)


# ---- C: export ---------------------------------------------------------------------------------------------------------
SHAPES_C = [('', (16, 24)), ('_odd', (5, 7))]


@pytest.mark.parametrize('tag,hw', SHAPES_C)
def test_export_equals_restatement_and_fixture(tag, hw):
    """Every uint16 of every pixel: each operation is one correctly rounded fp32 operation on both sides."""
    from motionpriorcmax_amd.utils import dsec_flow_png16
    f = K.export_flow(2, *hw)
    d = _dev(f)
    with _no_sync():
        out = dsec_flow_png16(d)
        one = dsec_flow_png16(d[1], max_magnitude=60)
    assert out.dtype == torch.uint16 and out.shape == (2,) + hw + (3,) and one.shape == hw + (3,)
    got = _u16(out)
    assert np.array_equal(got, K.export(f))
    assert np.array_equal(_u16(one), got[1])
    g = K.load('g20_dsec_export')
    assert np.array_equal(g['flow' + tag], f) and np.array_equal(got, g['png16' + tag])
    assert not got[..., 2].any()
    assert torch.equal(d, _dev(f))          # the input is left as it was (the reference clamps in place)
    other = K.export(f, 25.0)
    assert np.array_equal(_u16(dsec_flow_png16(d, 25.0)), other) and not np.array_equal(other, got)


@pytest.mark.parametrize('hw', [(16, 24), (5, 7)])
def test_export_of_non_finite_pixels_and_saturation(hw):
    """UNPINNED, as the docstring states them: a pixel with a NaN or infinite component gets payload 0; a q outside [0, 65535]
    (max_magnitude >= 256) saturates.  The neighbours are what the restatement gives."""
    from motionpriorcmax_amd.utils import dsec_flow_png16
    f = K.export_flow(2, *hw)
    bad = [(np.nan, 1.0), (2.0, np.nan), (np.inf, 3.0), (-4.0, -np.inf), (np.inf, np.inf), (np.nan, np.inf)]
    w = hw[1]
    pix = [(2 + (3 * k) // w, (3 * k) % w) for k in range(len(bad))]
    clean = K.export(f)
    for (r, c), (u, v) in zip(pix, bad):
        f[:, 0, r, c] = u; f[:, 1, r, c] = v
    got = _u16(dsec_flow_png16(_dev(f)))
    for r, c in pix:
        assert not got[:, r, c].any()
        clean[:, r, c] = 0
    assert np.array_equal(got, clean) and not got[..., 2].any()
    big = np.zeros((1, 2) + hw, np.float32)
    big[0, 0, 0, 0], big[0, 1, 0, 0] = 1e4, -1e4
    big[0, 0, 0, 1], big[0, 1, 0, 1] = -256.0, 255.9921875          # q = 0 and 65535 exactly: the ends of the range
    big[0, 0, 0, 2], big[0, 1, 0, 2] = -256.0078125, 256.0          # q = -1 and 65536: one step outside
    sat = _u16(dsec_flow_png16(_dev(big), max_magnitude=1e5))
    assert tuple(sat[0, 0, 0]) == (0, 65535, 0) and tuple(sat[0, 0, 1]) == (65535, 0, 0) and tuple(sat[0, 0, 2]) == (65535, 0, 0)
    assert (sat[0, 1:, :, :2] == 32768).all()


@pytest.mark.parametrize('hw', [(16, 24), (5, 7)])
def test_export_round_trip(hw):
    """decode(encode(f)) channel for channel in the (y, x) order of the flow: a swapped channel order on either side shows.
    The payload is trunc(c * 128 + 32768) for the clamped component c, which for a negative c is the floor of c * 128 and not its
    truncation, so the decoded value is (trunc(c * 128 + 32768) - 32768) / 128: at most 1 / 128 (plus the rounding of the fp32
    sum, 1 / 256 at 32768) below c, never above it by more than that rounding."""
    from motionpriorcmax_amd.utils import dsec_flow_png16, dsec_flow_targets
    f = K.export_flow(2, *hw)
    back = dsec_flow_targets(dsec_flow_png16(_dev(f)))
    c = K.clamp(f)
    want = (np.trunc(c * np.float32(128) + np.float32(32768)) - np.float32(32768)) / np.float32(128)
    got = back['forward_flow'].cpu().numpy()
    assert np.array_equal(got, want.astype(np.float32))
    assert not np.array_equal(got, want[:, ::-1])
    diff = c.astype(np.float64) - got
    assert diff.max() < 1 / 128 + 1 / 256 and diff.min() >= -1 / 256
    assert not back['flow_valid'].any()          # channel 2 of a submission is 0
