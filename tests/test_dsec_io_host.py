"""The restatements of tests/dsec_io_cases.py against the fixtures the unmodified reference produced (tests/golden/g20_dsec_*.npz,
tools/gen_golden_dsec_io.py), exactly; the cases carry what they are built for; the binding declares the new symbols.  No GPU."""
import numpy as np
import pytest

import dsec_io_cases as K


@pytest.fixture(scope='module')
def sample():
    return K.load('g20_dsec_sample')


@pytest.fixture(scope='module')
def exported():
    return K.load('g20_dsec_export')


def test_fixture_inputs_are_the_cases(sample, exported):
    """The fixtures hold the inputs the builders give: a test may rebuild them instead of loading them."""
    x, y, t, p, counts = K.raw_window()
    assert np.array_equal(sample['rectify_map'], K.rectify_map(), equal_nan=True)
    assert np.array_equal(sample['x'], x) and np.array_equal(sample['y'], y) and np.array_equal(sample['t'], t)
    assert np.array_equal(sample['p'], p) and np.array_equal(sample['counts'], counts) and int(sample['num_bins']) == K.NB
    assert np.array_equal(sample['png16'], K.payload(len(counts), K.H, K.W))
    assert np.array_equal(exported['flow'], K.export_flow(2, 16, 24)) and np.array_equal(exported['flow_odd'], K.export_flow(2, 5, 7))


def test_rectified_events_restatement_equals_reference(sample):
    """loader.py:152-167 + 360-415 behind the gather of :153."""
    m = sample['rectify_map']
    x, y = sample['x'].astype(np.int32), sample['y'].astype(np.int32)
    ev, num_pos = K.reference_events(m, x, y, sample['t'], sample['p'].astype(np.float32), sample['counts'], K.H, K.W, K.NB)
    assert num_pos == int(sample['num_pos_events'])
    assert np.array_equal(ev, sample['events'])


def test_rectification_case_leaves_the_image_on_all_sides_and_visits_the_planted_entries(sample):
    m = K.rectify_map()
    x, y, _, _, counts = K.raw_window()
    xr, yr = K.gather(m, x[0, :counts[0]], y[0, :counts[0]])
    with np.errstate(invalid='ignore'):
        assert (xr < 0).any() and (xr >= K.W).any() and (yr < 0).any() and (yr >= K.H).any()
        inside = (0 <= yr) & (yr < K.H) & (0 <= xr) & (xr < K.W)
    dist = np.abs(m - np.stack(np.meshgrid(np.arange(K.W), np.arange(K.H)), -1))
    for py, px in K.PLANTED:
        dist[py, px] = 0
    assert 2.0 < dist.max() <= 3.0 + 1e-5          # the smooth part: up to +-3 px
    planted = {(py, px): bool(inside[k]) for k, (py, px) in enumerate(K.PLANTED)}
    c = K.H // 2
    # 0.0 and -0.0 pass `0 <=`; W fails `< width`, the float below passes; NaN and +inf are dropped
    assert planted == {(c, 10): True, (c, 11): True, (c, 12): False, (c, 13): True, (c, 14): False, (c, 15): False,
                       (c, 16): True, (c, 17): True}
    assert np.signbit(m[c, 11, 0]) and m[c, 13, 0] < K.W and np.isnan(m[c, 14, 0]) and np.isposinf(m[c, 15, 1])


def test_decode_restatement_equals_reference(sample):
    """loader.py:174-180."""
    flow, valid = K.decode(sample['png16'])
    assert flow.dtype == np.float32 and valid.dtype == np.bool_
    assert np.array_equal(flow, sample['forward_flow']) and np.array_equal(valid, sample['flow_valid'])
    assert set(np.unique(sample['png16'][..., 2])) == {0, 1, 2, 255}
    assert valid[sample['png16'][..., 2] == 2].all() and valid[sample['png16'][..., 2] == 255].all()          # astype(bool), not == 1
    assert flow.min() == -256.0 and flow.max() == (65535 - 32768) / 128


@pytest.mark.parametrize('tag', ['', '_odd'])
def test_export_restatement_equals_reference(exported, tag):
    """dsec_inference.py:33-49; both branches of the clamp carry weight and the planted pixels do what they are for."""
    f, png = exported['flow' + tag], exported['png16' + tag]
    assert np.array_equal(K.export(f), png)
    assert not png[..., 2].any()
    mag = np.hypot(f[:, 0].astype(np.float64), f[:, 1].astype(np.float64))
    assert 0.2 < (mag > 60).mean() < 0.45
    w = f.shape[-1]
    px = lambda k: png[0, k // w, k % w]
    assert tuple(px(0)) == (32768 + 48 * 128, 32768 + 36 * 128, 0)          # (36, 48): magnitude exactly 60, not clamped; channel 0 = x
    assert tuple(px(5)) == (32768, 32768, 0) and tuple(px(9)) == (32768, 32768, 0)          # zeros, denormals
    clamped = K.clamp(f)
    assert np.array_equal(clamped[:, :, 0, 0], f[:, :, 0, 0]) and not np.array_equal(clamped[:, :, 0, 2], f[:, :, 0, 2])
    q7 = px(7).astype(np.int64) - 32768                                    # (1e4, -1e4) -> 60 / sqrt(2) each way
    assert abs(q7[1] - 5430) <= 1 and abs(q7[0] + 5430) <= 2


def test_flow_error64_agrees_with_the_fp32_oracle(sample):
    """The float64 yardstick of the GPU test against the project's fp32 restatement of the same lines (oracle/flow_oracle.py)."""
    from oracle import flow_oracle as F
    gt, valid = sample['forward_flow'][:2], sample['flow_valid'][:2]
    pr = K.prediction(gt)
    ts = np.array([[0.7], [1.3]], np.float32)
    a, b = K.flow_error64(gt, pr, valid, ts), F.calculate_flow_error(gt, pr, valid, ts)
    for k in K.FE_KEYS:
        assert abs(a[k] - float(b[k])) <= K.FE_RTOL * abs(a[k]), k
        assert a[k] > 0
    assert 0.05 < a['3PE'] < a['1PE'] < 0.95


def test_binding_declares_the_new_symbols():
    from motionpriorcmax_amd import _lib as C
    for name in ('mpc_ingest_rect_count', 'mpc_ingest_rect_scatter', 'mpc_ingest_rect_scatter_ordered', 'mpc_dsec_flow_decode',
                 'mpc_dsec_flow_error_workspace_bytes', 'mpc_dsec_flow_error', 'mpc_dsec_flow_encode'):
        assert name in C.EXPORTS
        assert hasattr(C.lib(), name)
    assert C.lib().mpc_version() == 107
