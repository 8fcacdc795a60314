"""CPU: the numpy restatement of the EVIMO2 / MultiFlow loss-event ingest (tests/ingest_window_oracle.py) against the fixtures the
unmodified reference produced (tools/gen_golden_window.py), bit for bit; and the argument checks of the host wrapper."""
import numpy as np
import pytest
import torch

import ingest_window_oracle as W


@pytest.mark.parametrize('name,split', [('g14_window_evimo2_split', True), ('g14_window_evimo2_single', False)])
def test_evimo2_restatement_equals_the_reference(name, split):
    g = W.load_window(name)
    ev, num_pos = W.restate('evimo2', g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']),
                            flow_duration_ms=int(g['flow_duration_ms']), polarity_aware_batching=split)
    assert num_pos == int(g['num_pos_events']) and (num_pos >= 0) == split
    np.testing.assert_array_equal(ev, g['events'])
    # the fixture tells fp32 from float64 in every sample (asserted by the generator, recorded in the file)
    assert ((g['n_differs'] > 0) | (g['kept'] != g['kept64'])).all()
    # the stamps lie where the two arithmetics part: at or above 100 s
    assert int(g['t_us'][0, 0]) >= 100_000_000


def test_multiflow_restatement_equals_the_reference():
    g = W.load_window('g14_window_multiflow')
    a = (g['x'], g['y'], g['t_us'], g['p'], g['counts'], int(g['num_bins']))
    ev, num_pos = W.restate('multiflow', *a, polarity_aware_batching=True)
    assert num_pos == int(g['num_pos_events'])
    np.testing.assert_array_equal(ev, g['events'])
    ev, num_pos = W.restate('multiflow', *a, polarity_aware_batching=False)
    assert num_pos == int(g['num_pos_events_single']) == -1
    np.testing.assert_array_equal(ev, g['events_single'])


def test_multiflow_restatement_is_the_dsec_arithmetic_without_the_filter():
    """sample.py:224-236 is loader.py:152-167 minus the in-image filter: the DSEC oracle with the filter opened up agrees."""
    from oracle import ingest_oracle as I
    g = W.load_window('g14_window_multiflow')
    n = int(g['counts'][0])
    a = (g['x'][0, :n], g['y'][0, :n], g['t_us'][0, :n], g['p'][0, :n])
    pos, neg = I.sample_events(*a, 1 << 30, 1 << 30, int(g['num_bins']))
    ours = W.multiflow_sample(*a, int(g['num_bins']))
    np.testing.assert_array_equal(pos, ours[ours[:, 3] == 1])
    np.testing.assert_array_equal(neg, ours[ours[:, 3] == 0])


def test_fixture_files_are_small():
    import os
    largest = max(os.path.getsize(os.path.join(W.GOLDEN, f)) for f in os.listdir(W.GOLDEN) if not f.startswith('g14_window_'))
    for name in W.FIXTURES:
        assert os.path.getsize(os.path.join(W.GOLDEN, name + '.npz')) < largest


def test_wrapper_rejects_bad_arguments_on_the_host():
    from motionpriorcmax_amd.utils import ingest_raw_events
    x = torch.zeros((1, 8), dtype=torch.int32)
    t = torch.arange(8, dtype=torch.int64)[None]
    p = torch.zeros((1, 8), dtype=torch.int64)
    cnt = torch.tensor([8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ingest_raw_events(x, x, t, p, cnt, 41, 'evimo2', flow_duration_ms=300)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ingest_raw_events(x, x, t, p, cnt, 41, 'multiflow')
    with pytest.raises(ValueError, match='flow_duration_ms'):
        ingest_raw_events(x, x, t, p, cnt, 41, 'evimo2')
    with pytest.raises(ValueError, match='flow_duration_ms'):
        ingest_raw_events(x, x, t, p, cnt, 41, 'multiflow', flow_duration_ms=300)
    with pytest.raises(ValueError, match='dataset'):
        ingest_raw_events(x, x, t, p, cnt, 41, 'dsec')


def test_window_shape_validation_is_host_only():
    import ctypes
    from motionpriorcmax_amd import _lib as C
    ok = dict(B=2, N=100, nb=41, time_mode=C.WINDOW_TIME_FP32_SUFFIX, xy_int=1, p_int64=1, split=1, duration_us=3e5, x_scale=1, y_scale=1)
    n1 = C.lib().mpc_ingest_window_workspace_bytes(ctypes.byref(C.WindowShape(**ok)))
    assert n1 > 0
    assert C.lib().mpc_ingest_window_workspace_bytes(ctypes.byref(C.WindowShape(**dict(ok, time_mode=2)))) == C.E_SHAPE
    assert C.lib().mpc_ingest_window_workspace_bytes(ctypes.byref(C.WindowShape(**dict(ok, nb=0)))) == C.E_SHAPE
    assert C.lib().mpc_ingest_window_workspace_bytes(ctypes.byref(C.WindowShape(**dict(ok, nb=4096)))) == C.E_UNSUPPORTED
    assert C.lib().mpc_ingest_window_workspace_bytes(ctypes.byref(C.WindowShape(**dict(ok, nb=4096, time_mode=C.WINDOW_TIME_MINMAX64)))) > 0
    assert C.lib().mpc_ingest_window_count(ctypes.byref(C.WindowShape(**ok)), None, None, None, None, None, None) == C.E_NULL
