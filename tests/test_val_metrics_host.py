"""The RAFT-spline validation metrics on the host: the float64 restatement of tests/val_metrics_oracle.py against the g15_val fixtures
(tools/gen_golden_val.py: the unmodified reference's functions in fp32, the same chain in float64 and the distance between the two),
the C ABI of the new entry points, and the argument errors of utils.trajectory_val_metrics, each raised before any GPU call.

Tolerance rule (tests/test_cvx_traj_host.py, shared with tests/test_gpu_val_metrics.py): |x - x_f64| <= max(4 * err_x, 2^-22 * |x_f64|)
with err_x the reference's own fp32 error from the fixture; NaN must meet NaN and the `updated` flags must be equal.  The fixtures keep
every pixel off the thresholds of the count metrics (the generator asserts the margins), so those are exact.  Every figure is printed
before it is asserted (pytest -s shows them)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import val_metrics_oracle as O
from conftest import ROOT, load_golden

CASES = ['a', 'b', 'c', 'd', 'e']


def load_case(case):
    g = load_golden('g15_val_' + case)
    if 'pred' not in g:
        g['pred'] = load_golden(f'g15_val_{case}_pred')['pred']
    g['keys'] = [str(k) for k in g['keys']]
    return g


def check_against_fixture(label, g, values, updated):
    """values / updated: dicts over the logged names (anything float() / int() takes)."""
    assert sorted(values) == sorted(g['keys']) and sorted(updated) == sorted(g['keys'])
    worst = 0.0
    for i, k in enumerate(g['keys']):
        want, got, bound = float(g['f64'][i]), float(values[k]), O.bound(float(g['f64'][i]), float(g['err'][i]))
        print(f'{label} {k}: {got!r} vs {want!r}  |diff| {abs(got - want):.3g} (bound {bound:.3g})  updated {int(updated[k])} vs {int(g["updated"][i])}')
        assert int(updated[k]) == int(g['updated'][i]), (label, k)
        if np.isnan(want):
            assert np.isnan(got), (label, k, got)
        else:
            assert abs(got - want) <= bound, (label, k, got, want, bound)
            worst = max(worst, abs(got - want) / bound if bound else 0.0)
    return worst


def oracle_inputs(g, dtype):
    pred = torch.from_numpy(g['pred']).to(dtype)
    if dtype == torch.float64 and 'params' in g:
        pred = O.curve_flows(torch.from_numpy(g['params']).double(), torch.from_numpy(g['mask']).double(), g['times'], float(g['scale']))
    valid = torch.from_numpy(g['flow_valid']) if 'flow_valid' in g else None
    return pred, torch.from_numpy(g['flow_gt']).to(dtype), g['times'], valid, O.event_mask(torch.from_numpy(g['ev_repr']))


@pytest.mark.parametrize('case', CASES)
def test_restatement_matches_the_fixtures(case):
    g = load_case(case)
    M = len(g['times'])
    assert len(g['keys']) == 12 + 3 * (5 + M)
    values, updated = O.metrics(*oracle_inputs(g, torch.float64))
    check_against_fixture(f'{case} f64', g, values, updated)
    # the same code in fp32 on the reference's own predictions: the margins the generator asserts keep every count as it is
    values32, updated32 = O.metrics(*oracle_inputs(g, torch.float32))
    assert updated32 == updated
    for k in g['keys']:
        if k.endswith(('1pe', '2pe', '3pe', 'T3PE')) and not np.isnan(values[k]):
            assert values32[k] == values[k], (k, values32[k], values[k])


@pytest.mark.parametrize('case', CASES)
def test_the_fixtures_hold_what_the_cases_are_for(case):
    g = load_case(case)
    gt, names = g['flow_gt'], g['keys']
    assert ((gt[:, :, 0] == 0) ^ (gt[:, :, 1] == 0)).any() and ((gt[:, :, 0] == 0) & (gt[:, :, 1] == 0)).any()
    pred64 = oracle_inputs(g, torch.float64)[0]
    assert not O.threshold_violations(pred64, torch.from_numpy(gt).double()).any()
    val = dict(zip(names, g['f64']))
    upd = dict(zip(names, g['updated']))
    assert ('flow_valid' in g) == (case != 'b') and ('params' in g) == (case != 'd')
    if case == 'a':
        assert np.isnan(g['ev_repr']).sum() == 1
    if case == 'c':
        assert not g['flow_valid'][:, 2].any() and g['flow_valid'][1].sum() == 15 and gt.shape[-1] == 264
        assert np.isnan(val['val/masked_ae_multi']) and np.isfinite(val['val/masked_epe_multi']) and upd['val/masked_epe_multi'] == 1
        assert abs(val['val/masked_TEPE'] - val['val/masked_epe_multi']) > 1e-2          # per-image against per-batch normalisation
    if case == 'd':
        assert gt.shape[-2:] == (13, 21) and len(g['times']) == 3
    if case == 'e':
        assert not g['ev_repr'].any()
        assert all(np.isnan(val['val/masked_' + k]) and upd['val/masked_' + k] == 0 for k in O.SINGLE)
        assert np.isnan(val['val/ev_masked_epe_multi']) and upd['val/ev_masked_epe_multi'] == 0
        assert np.isnan(val['val/ev_masked_ae_multi']) and upd['val/ev_masked_ae_multi'] == 1
        assert val['val/ev_masked_TEPE'] == 0.0 and upd['val/ev_masked_TEPE'] == 1


def test_the_key_order_of_the_package_covers_the_fixture_names():
    from motionpriorcmax_amd import _lib, utils
    for case in ('a', 'd'):
        g = load_case(case)
        keys = utils.val_metric_keys(len(g['times']))
        assert sorted(k for k, _ in keys) == sorted(g['keys'])
        idx = [i for _, i in keys]
        assert len(set(idx)) == len(idx) and max(idx) < _lib.VAL_COUNT
    src = open(os.path.join(ROOT, 'include', 'mpcmax.h')).read()
    macros = {m: int(v) for m, v in re.findall(r'#define (MPC_VAL_[A-Z_0-9]+) (\d+)', src)}
    assert macros['MPC_VAL_COUNT'] == _lib.VAL_COUNT and macros['MPC_VAL_MAX_STEPS'] == _lib.VAL_MAX_STEPS
    assert (macros['MPC_VAL_MASKED_SINGLE'], macros['MPC_VAL_MULTI'], macros['MPC_VAL_EV_MASKED_MULTI'], macros['MPC_VAL_MASKED_MULTI'],
            macros['MPC_VAL_EPE_MULTI_LIN'], macros['MPC_VAL_AE_MULTI_LIN']) == \
        (_lib.VAL_MASKED_SINGLE, _lib.VAL_MULTI, _lib.VAL_EV_MASKED_MULTI, _lib.VAL_MASKED_MULTI, _lib.VAL_EPE_MULTI_LIN, _lib.VAL_AE_MULTI_LIN)
    assert macros['MPC_VAL_EV_MASKED_MULTI'] - macros['MPC_VAL_MULTI'] == 5 + macros['MPC_VAL_MAX_STEPS'] == macros['MPC_VAL_EPE_MULTI_LIN'] - macros['MPC_VAL_MASKED_MULTI']
    assert [macros['MPC_VAL_' + k.upper()] for k in _lib.VAL_SINGLE_KEYS] == [0, 1, 2, 3, 4]
    assert [macros['MPC_VAL_' + k.upper()] for k in _lib.VAL_MULTI_KEYS] + [macros['MPC_VAL_EPE_STEP']] == [0, 1, 2, 3, 4, 5]


def test_the_library_exports_the_two_entry_points():
    from motionpriorcmax_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mpc_val_metrics_workspace_bytes', 'mpc_val_metrics'):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert _lib.lib().mpc_version() == 107


def test_limits_and_workspace_size_are_host_only():
    from motionpriorcmax_amd import _lib
    L = _lib.lib()

    def nbytes(**kw):
        d = dict(B=2, M=6, d=10, h=3, w=4, H=24, W=32, C=5)
        d.update(kw)
        return L.mpc_val_metrics_workspace_bytes(ctypes.byref(_lib.ValShape(**d)))
    assert nbytes() > 0 and nbytes(B=4) > nbytes() and nbytes(C=0) < nbytes(C=5, H=240, W=320, h=30, w=40)
    assert nbytes(M=17) == _lib.E_UNSUPPORTED and nbytes(d=17) == _lib.E_UNSUPPORTED
    assert nbytes(M=16, d=16) > 0 and nbytes(d=0, H=13, W=21) > 0
    assert nbytes(H=25) == _lib.E_SHAPE and nbytes(M=0) == _lib.E_SHAPE
    shape = _lib.ValShape(B=0, M=6, d=10, h=3, w=4, H=24, W=32, C=5)
    assert L.mpc_val_metrics(ctypes.byref(shape), *([None] * 4), 1.0, *([None] * 9)) == 0           # B = 0 launches nothing
    shape.B = 1
    assert L.mpc_val_metrics(ctypes.byref(shape), *([None] * 4), 1.0, *([None] * 9)) == _lib.E_NULL


def test_argument_errors_come_before_any_gpu_call():
    """CPU tensors throughout: a ValueError here was raised before anything asked for the device (which raises RuntimeError)."""
    from motionpriorcmax_amd import utils
    B, M, h, w = 1, 6, 2, 3
    gt, ts = torch.zeros(B, M, 2, 8 * h, 8 * w), torch.linspace(0.1, 1.0, M)
    p, m = torch.zeros(B, 8, h, w), torch.zeros(B, 576, h, w)
    flows, ev, em = torch.zeros(M, B, 2, 8 * h, 8 * w), torch.zeros(B, 3, 8 * h, 8 * w), torch.zeros(B, 8 * h, 8 * w, dtype=torch.bool)
    f = utils.trajectory_val_metrics
    for kw in (dict(ev_repr=ev),                                             # no prediction source
               dict(params=p, up_mask=m, flows=flows, ev_repr=ev),           # both
               dict(flows=flows),                                            # no mask source
               dict(flows=flows, ev_repr=ev, event_mask=em),                 # both
               dict(params=p, up_mask=m[:, :64], ev_repr=ev),                # a wrong up_mask
               dict(params=p, ev_repr=ev),
               dict(params=p[:, :, :1], up_mask=m[:, :, :1], ev_repr=ev),    # a grid that is not 1/8 of the ground truth
               dict(flows=flows[:, :, :, :-1], ev_repr=ev),
               dict(flows=flows, ev_repr=ev, flow_valid=torch.ones(B, M - 1, 8 * h, 8 * w, dtype=torch.bool))):
        with pytest.raises(ValueError):
            f(gt, ts, **kw)
    with pytest.raises(ValueError):                                          # M > 16
        f(torch.zeros(B, 17, 2, 8, 8), torch.linspace(0, 1, 17), flows=torch.zeros(17, B, 2, 8, 8), ev_repr=torch.zeros(B, 1, 8, 8))
    with pytest.raises(ValueError):
        f(gt, ts[:-1], flows=flows, ev_repr=ev)
    with pytest.raises(ValueError):
        utils.TrajectoryValMetrics().update(gt, ts, ev_repr=ev)
    with pytest.raises(RuntimeError):                                        # CPU tensors raise, as everywhere in the package
        f(gt, ts, flows=flows, ev_repr=ev)
    with pytest.raises(RuntimeError):
        f([g for g in gt.unbind(1)], ts, params=p, up_mask=m, event_mask=em)
