"""The RAFT-spline validation metrics on the device: utils.trajectory_val_metrics / utils.TrajectoryValMetrics (csrc/val_metrics.hip:
mpc_val_metrics) against the g15_val fixtures of the unmodified reference (tools/gen_golden_val.py) and the float64 restatement of
tests/val_metrics_oracle.py, at the rule of tests/test_val_metrics_host.py: |x_gpu - x_f64| <= max(4 * err_x, 2^-22 * |x_f64|) with
err_x the reference's own fp32 error from the fixture, NaN meets NaN, `updated` equal.  Every figure is printed before it is asserted
(pytest -s shows them)."""
import numpy as np
import pytest
import torch

import val_metrics_oracle as O
from test_val_metrics_host import CASES, check_against_fixture, load_case

pytestmark = pytest.mark.gpu
CURVE_CASES = [c for c in CASES if c != 'd']


def _dev():
    return torch.device('cuda', 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _common(g):
    kw = dict(ev_repr=_t(g['ev_repr']))
    if 'flow_valid' in g:
        kw['flow_valid'] = _t(g['flow_valid'])
    return _t(g['flow_gt']), g['times'], kw


def _curves(g):
    return dict(params=_t(g['params']), up_mask=_t(g['mask']), scale=float(g['scale']))


def _host(d):
    return {k: v.item() for k, v in d.items()}


def _bitwise(a, b):
    """Two (values, updated) results: the same bits (NaN included)."""
    assert list(a[0]) == list(b[0])
    for k in a[0]:
        assert torch.equal(a[0][k].view(torch.int32), b[0][k].view(torch.int32)), k
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize('case', CURVE_CASES)
def test_fixtures_in_curves_mode(case):
    from motionpriorcmax_amd import ops, utils
    g = load_case(case)
    gt, times, kw = _common(g)
    with ops.KernelTimer() as kt:
        values, updated = utils.trajectory_val_metrics(gt, times, **_curves(g), **kw)
    launches = {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}
    assert launches == {'k_val_evmask': 1, 'k_val_partial': 1, 'k_val_image': 1, 'k_val_final': 1}, launches
    v = next(iter(values.values()))
    assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 0 and next(iter(updated.values())).dtype == torch.int32
    check_against_fixture(f'{case} curves', g, _host(values), _host(updated))


@pytest.mark.parametrize('case', CASES)
def test_fixtures_in_flows_mode(case):
    """Fed the reference's own fp32 predictions (they carry the fixture's scale already); the ground truth as a list of steps."""
    from motionpriorcmax_amd import utils
    g = load_case(case)
    gt, times, kw = _common(g)
    values, updated = utils.trajectory_val_metrics(list(gt.unbind(1)), times, flows=_t(g['pred']), **kw)
    check_against_fixture(f'{case} flows', g, _host(values), _host(updated))


@pytest.mark.parametrize('case', CURVE_CASES)
def test_the_two_modes_agree(case):
    """`flows` mode fed by flows_from_bezier: the same device functions evaluate the curves, so the same bits are expected; the
    rule is what is required."""
    from motionpriorcmax_amd import utils
    g = load_case(case)
    gt, times, kw = _common(g)
    c = _curves(g)
    a = utils.trajectory_val_metrics(gt, times, **c, **kw)
    flows = utils.flows_from_bezier(c['params'], times, up_mask=c['up_mask'], scale=c['scale'])
    b = utils.trajectory_val_metrics(gt, times, flows=flows, **kw)
    check_against_fixture(f'{case} flows_from_bezier', g, _host(b[0]), _host(b[1]))
    _bitwise(a, b)


def _random_batch(seed, B=2, h=8, w=12, d=10, C=9, M=6):
    gen = torch.Generator().manual_seed(seed)
    times = np.asarray([0.15, 0.3, 0.5, 0.65, 0.85, 1.0]) if M == 6 else np.arange(1, M + 1) / M
    P = torch.randn(B, 2 * d, h, w, generator=gen) * 0.5
    Mk = torch.randn(B, 576, h, w, generator=gen) * 2.0
    pred64 = O.curve_flows(P.double(), Mk.double(), times)
    H, W = 8 * h, 8 * w
    mag = torch.exp(torch.rand(B, M, H, W, generator=gen) * (np.log(6.0) - np.log(0.02)) + np.log(0.02))
    ang = torch.rand(B, M, H, W, generator=gen) * (2 * np.pi)
    gt = (pred64.permute(1, 0, 2, 3, 4) + torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=2)).float()
    kind = torch.rand(B, M, H, W, generator=gen)
    gt[:, :, 0][kind < 0.03] = 0.0
    gt[:, :, 1][(kind >= 0.03) & (kind < 0.06)] = 0.0
    gt[((kind >= 0.06) & (kind < 0.1))[:, :, None].expand_as(gt)] = 0.0
    gt = O.push_off_thresholds(pred64, gt)
    ev = torch.randn(B, C, H, W, generator=gen) * (torch.rand(B, C, H, W, generator=gen) < 0.1)
    valid = torch.rand(B, M, H, W, generator=gen) < 0.7
    return P, Mk, times, gt, ev, valid, pred64


def _against_the_restatement(label, batch, n_keys):
    from motionpriorcmax_amd import utils
    P, Mk, times, gt, ev, valid, pred64 = batch
    E = O.event_mask(ev)
    want, want_up = O.metrics(pred64, gt.double(), times, valid, E)
    pred32 = utils.flows_from_bezier(P, times, up_mask=Mk)                      # CPU tensors: the plain-torch mirror
    v32, _ = O.metrics(pred32, gt, times, valid, E)
    args = (gt.to(_dev()), times)
    kw = dict(flow_valid=valid.to(_dev()), ev_repr=ev.to(_dev()))
    curves = utils.trajectory_val_metrics(*args, params=P.to(_dev()), up_mask=Mk.to(_dev()), **kw)
    flows = utils.trajectory_val_metrics(*args, flows=utils.flows_from_bezier(P.to(_dev()), times, up_mask=Mk.to(_dev())), **kw)
    _bitwise(curves, flows)
    values, updated = _host(curves[0]), _host(curves[1])
    assert updated == want_up and len(values) == n_keys
    for k, x in want.items():
        bound = O.bound(x, abs(v32[k] - x))
        print(f'{label} {k}: {values[k]!r} vs {x!r}  |diff| {abs(values[k] - x):.3g} (bound {bound:.3g})')
        assert abs(values[k] - x) <= bound, (k, values[k], x, bound)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_batches_against_the_restatement(seed):
    """B = 2, 64 x 96 (six workgroups a sample), C = 9, both modes: the float64 restatement is the oracle.  No fixture recorded the
    reference's fp32 error here; in its place stands the distance between the restatement run in fp32 on the package's plain-torch
    fp32 curves (the reference's operations at the reference's precision) and in float64 -- one draw of the same noise, with the
    rule's floor of fp32 output rounding under it.  The ground truth is pushed off the count thresholds as the generator does."""
    _against_the_restatement(f'seed {seed}', _random_batch(seed), 45)


@pytest.mark.parametrize('M', [1, 8, 16])
def test_other_step_counts_against_the_restatement(M):
    """The kernel parks 2 M floats a pixel in LDS and takes fewer pixels a thread as M grows (4 up to M = 7, 3 at M = 8, 1 at M = 16):
    every such size, at 16 x 40 pixels (one to three workgroups), d = 3, under the rule of the random batches."""
    _against_the_restatement(f'M {M}', _random_batch(10 + M, B=1, h=2, w=5, d=3, C=2, M=M), 12 + 3 * (5 + M))


def test_event_mask_in_the_place_of_ev_repr_and_two_calls_are_bitwise_equal():
    from motionpriorcmax_amd import utils
    g = load_case('c')
    gt, times, kw = _common(g)
    a = utils.trajectory_val_metrics(gt, times, **_curves(g), **kw)
    b = utils.trajectory_val_metrics(gt, times, **_curves(g), **kw)
    _bitwise(a, b)
    em = O.event_mask(torch.from_numpy(g['ev_repr'])).to(_dev())
    c = utils.trajectory_val_metrics(gt, times, **_curves(g), flow_valid=kw['flow_valid'], event_mask=em)
    _bitwise(a, c)
    g = load_case('a')                                                          # the NaN of case a's ev_repr counts as an event
    gt, times, kw = _common(g)
    em = O.event_mask(torch.from_numpy(g['ev_repr'])).to(_dev())
    assert bool(em[0, 3, 5])
    _bitwise(utils.trajectory_val_metrics(gt, times, **_curves(g), **kw),
             utils.trajectory_val_metrics(gt, times, **_curves(g), flow_valid=kw['flow_valid'], event_mask=em))


def test_accumulator_over_two_batches():
    """Cases a and c as two batches: per key the reference's per-batch values (float64) combined by the Metric rule -- the sum of the
    values its update() adds over their number.  The bound is the rule on the combined value, with the mean of the two batches'
    recorded errors as err_x (the error of a mean of two is at most the mean of their errors)."""
    from motionpriorcmax_amd import utils
    acc = utils.TrajectoryValMetrics()
    batches = []
    for case in ('a', 'c'):
        g = load_case(case)
        gt, times, kw = _common(g)
        acc.update(gt, times, **_curves(g), **kw)
        batches.append(g)
    sums, totals = acc.state()
    assert sums.dtype == torch.float64 and totals.dtype == torch.int64 and sums.is_cuda and sums.shape == totals.shape == (75,)
    got = _host(acc.compute())
    names = batches[0]['keys']
    assert sorted(got) == sorted(names)
    for k in names:
        i, j = names.index(k), batches[1]['keys'].index(k)
        parts = [(float(g['f64'][n]), float(g['err'][n])) for g, n in ((batches[0], i), (batches[1], j)) if int(g['updated'][n])]
        assert len(parts) == 2                                              # (nothing of a or c is skipped)
        want, err = sum(p[0] for p in parts) / 2, sum(p[1] for p in parts) / 2
        print(f'{k}: {got[k]!r} vs {want!r} (bound {O.bound(want, err) if not np.isnan(want) else float("nan"):.3g})')
        if np.isnan(want):
            assert np.isnan(got[k]), k                                      # a NaN the reference adds is added
        else:
            assert abs(got[k] - want) <= O.bound(want, err), (k, got[k], want)
    assert int(totals[0]) == 2
    acc.reset()
    with pytest.raises(RuntimeError):
        acc.state()


def test_an_empty_mask_is_skipped_by_the_accumulator():
    """Case e (no event) then case a: the keys the reference skips in e count one batch, the others two."""
    from motionpriorcmax_amd import utils
    acc = utils.TrajectoryValMetrics()
    for case in ('e', 'a'):
        g = load_case(case)
        gt, times, kw = _common(g)
        acc.update(gt, times, **_curves(g), **kw)
    totals = dict(zip([k for k, _ in utils.val_metric_keys(6)], acc.state()[1][[i for _, i in utils.val_metric_keys(6)]].tolist()))
    ga = load_case('a')
    got = _host(acc.compute())
    for k in ('val/masked_epe', 'val/masked_3pe', 'val/ev_masked_epe_multi'):
        assert totals[k] == 1
        i = ga['keys'].index(k)
        assert abs(got[k] - float(ga['f64'][i])) <= O.bound(float(ga['f64'][i]), float(ga['err'][i])), k
    assert totals['val/epe'] == 2 and totals['val/ev_masked_TEPE'] == 2 and np.isnan(got['val/ev_masked_ae_multi'])


def test_capture_and_replay_give_the_same_numbers():
    """One stream, a single-branch graph: the four kernels captured and replayed."""
    from motionpriorcmax_amd import utils
    g = load_case('c')
    gt, times, kw = _common(g)
    c = _curves(g)
    ts = torch.tensor(times, dtype=torch.float32, device=_dev())                # a device tensor: the cached basis needs no upload
    eager = utils.trajectory_val_metrics(gt, ts, **c, **kw)
    eager = ({k: v.clone() for k, v in eager[0].items()}, {k: v.clone() for k, v in eager[1].items()})
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                  # warm-up outside the capture
        for _ in range(2):
            utils.trajectory_val_metrics(gt, ts, **c, **kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = utils.trajectory_val_metrics(gt, ts, **c, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _bitwise(static, eager)
    check_against_fixture('c replayed', g, _host(static[0]), _host(static[1]))


def test_no_host_synchronisation():
    from motionpriorcmax_amd import utils
    g = load_case('a')
    gt, times, kw = _common(g)
    c = _curves(g)
    ts = torch.tensor(times, dtype=torch.float32, device=_dev())
    acc = utils.TrajectoryValMetrics()
    acc.update(gt, ts, **c, **kw)                                               # warm-up: library load, cached basis
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        values, updated = utils.trajectory_val_metrics(gt, ts, **c, **kw)
        acc.update(gt, ts, **c, **kw)
        out = acc.compute()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert len(values) == len(out) == 45


def test_an_empty_batch_launches_nothing():
    from motionpriorcmax_amd import ops, utils
    dev = _dev()
    with ops.KernelTimer() as kt:
        values, updated = utils.trajectory_val_metrics(torch.zeros(0, 3, 2, 8, 16, device=dev), [0.2, 0.6, 1.0], flows=torch.zeros(3, 0, 2, 8, 16, device=dev),
                                                       event_mask=torch.zeros(0, 8, 16, dtype=torch.bool, device=dev))
    assert not [k for k in kt.summary() if k.startswith('k_val')]
    assert all(np.isnan(v.item()) for v in values.values()) and not any(u.item() for u in updated.values()) and len(values) == 36
