"""The voxel-grid builder (csrc/voxel.hip over csrc/strip_buckets.h) at its edges, against the float64 oracle
(oracle.voxel_oracle.voxel_grid64): the named cases of tests/voxel_cases.py -- spilled buckets under every normalisation and in
both samples of a batch, a short last strip with events on the seams, the wide-sensor LDS fallback, 1 x 1 x 1 up to 3 x 5 x 7
(integer quantile rank), tied and zero clipping thresholds, times outside [first, last] and unsorted, empty / one-event / over-long
samples, non-finite coordinates, all entries equal -- the reference's edge fixtures, run-to-run and batch bitwise equality, graph
capture without host synchronisation, and the error returns.

Every comparison uses the bound of tests/voxel_cases.py, max(4 err32, 2^-22 max |X_64|) + T 2^-30 m, no entry excused, and
entries that are zero in float64 must be +-0 on the device.  The figures are printed before they are asserted (pytest -s).

Measured on an MI355X: the worst ratio of a difference to its bound over the named cases is 0.378 (nonfinite, mean_std: 4.7e-7
against 1.24e-6), next time / max 0.337 and short_strip / max 0.309; the bounds run from 2.5e-7 to 2.1e-6; no entry that is zero in
float64 was non-zero on the device; the batch and run-to-run comparisons are bitwise.  104 tests in 1.5 s."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_cases as VC

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


def _run(case, norm, q):
    from motionpriorcmax_amd.utils import voxel_grids
    ev, cnt = case.batch()
    return voxel_grids(ev.to(_dev()), cnt.to(_dev()), case.shape, norm, q)


def _judge_all(out, exp, label):
    worst = 0.0
    for b, o in enumerate(exp):
        assert VC.input_caps(o) == (0, 0)                            # the caps on the inputs hold here as on the CPU
        ratio, nzz, bad = VC.judge(out[b], o, f'{label} sample {b}')
        assert bad == 0
        assert nzz == 0, 'an entry that is zero in float64 is not +-0 on the device'
        assert ratio <= 1.0
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('name,norm,q', VC.case_params())
def test_voxel_case_vs_float64(name, norm, q):
    case = VC.cases()[name]
    out = _run(case, norm, q).cpu()
    assert out.shape == (case.B,) + case.shape
    _judge_all(out, VC.expected(name, norm, q), f'{name} {norm} q={q}')
    if name == 'all_equal':
        assert float(out.abs().max()) <= 2e-6


@pytest.mark.parametrize('name', VC.EDGE_FIXTURES)
def test_voxel_edge_fixture(name):
    """The reference's own output for the edge windows, through VoxelGrid.convert: within the same bound, the reference's fp32
    grid standing in for the fp32 oracle (which tests/test_voxel_cases_host.py pins to it)."""
    from motionpriorcmax_amd.utils import VoxelGrid
    g, ev, shape, norm, q = VC.fixture(name)
    out = VoxelGrid(shape, norm_type=norm, quantile=q).convert({k: v.to(_dev()) for k, v in zip('xytp', ev)}).cpu()
    o = VC.oracles(ev, shape, norm, q)
    ratio, nzz, bad = VC.judge(out, o, name)
    assert bad == 0 and nzz == 0 and ratio <= 1.0
    np.testing.assert_allclose(out.numpy(), g['grid'], rtol=0, atol=2e-6 * max(1.0, np.abs(g['grid']).max()))     # (test_gpu_voxel.py's rule)
    if name != 'g8_voxel_e_time' and name != 'g8_voxel_e_int_q05':
        assert not out.any()                                         # (all-zero, finite grids: +-0 only)


@pytest.mark.parametrize('norm,q', [('mean_std', 0.0), ('mean_std', 0.05), (None, 0.05), ('max', 0.0)])
def test_voxel_spill_runs_are_bitwise_equal(norm, q):
    """Integer sums in LDS and a fixed reduction order: the spill batch (records land in the spill region in a different order
    every run) gives the same bits twice."""
    case = VC.cases()['spill']
    a, b = _run(case, norm, q), _run(case, norm, q)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0


@pytest.mark.parametrize('name,norm,q', [('spill', 'mean_std', 0.0), ('spill', None, 0.0), ('spill', 'mean_std', 0.05),
                                         ('ragged', 'mean_std', 0.0), ('ragged', 'max', 0.05)])
def test_voxel_sample_of_a_batch_equals_the_sample_alone(name, norm, q):
    from motionpriorcmax_amd.utils import voxel_grids
    case = VC.cases()[name]
    ev, cnt = case.batch()
    ev, cnt = ev.to(_dev()), cnt.to(_dev())
    full = voxel_grids(ev, cnt, case.shape, norm, q)
    for b in range(case.B):
        alone = voxel_grids(ev[b:b + 1].contiguous(), cnt[b:b + 1].contiguous(), case.shape, norm, q)
        assert torch.equal(alone[0], full[b]), b
    # ... and in another place of the batch, among other samples
    perm = list(reversed(range(case.B)))
    rev = voxel_grids(ev[perm].contiguous(), cnt[perm].contiguous(), case.shape, norm, q)
    assert torch.equal(rev, full[perm])


@pytest.mark.parametrize('norm,q', [('mean_std', 0.0), ('max', 0.05)])
def test_voxel_no_host_sync_and_graph_capture(norm, q):
    from motionpriorcmax_amd.utils import voxel_grids
    dev = _dev()
    case = VC.cases()['ragged']
    ev0, cnt0 = case.batch()
    ev, cnt = ev0.to(dev), cnt0.to(dev)
    voxel_grids(ev, cnt, case.shape, norm, q)                        # one-time set-up outside the checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        voxel_grids(ev, cnt, case.shape, norm, q)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    # capture once, then replay with refilled inputs
    fresh_ev = ev0.flip(0).contiguous()
    fresh_ev[..., 0] = (fresh_ev[..., 0] + 3.25) % case.shape[2]
    fresh = (fresh_ev.to(dev), torch.tensor([case.N, 7, case.N - 3, 0], dtype=torch.int32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside the capture
        voxel_grids(ev, cnt, case.shape, norm, q)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = voxel_grids(ev, cnt, case.shape, norm, q)
    for inputs in ((ev.clone(), cnt.clone()), fresh):
        eager = voxel_grids(*inputs, case.shape, norm, q)
        ev.copy_(inputs[0])
        cnt.copy_(inputs[1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        assert out.abs().sum() > 0


def test_voxel_error_returns_launch_nothing():
    from motionpriorcmax_amd import _lib as C, ops
    from motionpriorcmax_amd.utils import VoxelGrid, voxel_grids
    dev = _dev()
    L = C.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    grid = torch.full((64,), 7.0, device=dev)
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731

    def shape(**kw):
        d = dict(B=1, N=8, C=2, H=4, W=8, norm=0, quantile=0.0, keep=0.0)
        d.update(kw)
        return C.VoxShape(**d)

    def call(s, ev=buf, c=cnt, g=grid, ws=buf):
        return L.mpc_voxel_grid(ctypes.byref(s) if s is not None else None, p(ev) if ev is not None else None,
                                p(c) if c is not None else None, p(g) if g is not None else None,
                                p(ws) if ws is not None else None, None)

    with ops.KernelTimer() as kt:
        assert call(None) == C.E_NULL
        assert call(shape(), ev=None) == C.E_NULL
        assert call(shape(), c=None) == C.E_NULL
        assert call(shape(), g=None) == C.E_NULL
        assert call(shape(), ws=None) == C.E_NULL
        assert b'null' in L.mpc_last_error_string()
        assert L.mpc_voxel_workspace_bytes(None) == C.E_NULL
        for bad in (shape(C=0), shape(norm=3), shape(norm=-1), shape(quantile=0.15), shape(quantile=-0.01), shape(H=0), shape(N=-1)):
            assert call(bad) == C.E_SHAPE
            assert L.mpc_voxel_workspace_bytes(ctypes.byref(bad)) == C.E_SHAPE
        assert b'quantile' in L.mpc_last_error_string() or b'shape' in L.mpc_last_error_string()
        wide = shape(W=19201)
        assert call(wide) == C.E_UNSUPPORTED and L.mpc_voxel_workspace_bytes(ctypes.byref(wide)) == C.E_UNSUPPORTED
        assert b'wide' in L.mpc_last_error_string()
        assert L.mpc_voxel_workspace_bytes(ctypes.byref(shape(W=19200))) > 0
        big = shape(B=1, C=16, H=8192, W=16384)                      # B C H W = 2^31
        assert call(big) == C.E_UNSUPPORTED and L.mpc_voxel_workspace_bytes(ctypes.byref(big)) == C.E_UNSUPPORTED
        assert b'large' in L.mpc_last_error_string()
        assert call(shape(B=2, C=16, H=8192, W=8192)) == C.E_UNSUPPORTED
        assert call(shape(B=0)) == 0
        assert call(shape(B=0), ev=None) == 0
    assert kt.summary() == {}, kt.summary()
    assert bool((grid == 7.0).all())
    # the Python layer
    case = VC.cases()['time']
    ev, c = case.batch()
    with pytest.raises(RuntimeError, match='GPU tensor'):
        voxel_grids(ev, c, case.shape, None)
    with pytest.raises(AssertionError):
        voxel_grids(ev.to(dev), c, case.shape, 'l2')
    with pytest.raises(AssertionError):
        VoxelGrid(case.shape, norm_type='l2', quantile=0.0)
    with pytest.raises(AssertionError):
        VoxelGrid(case.shape, norm_type=None, quantile=0.15)
    with pytest.raises(RuntimeError, match='quantile'):
        voxel_grids(ev.to(dev), c, case.shape, None, 0.2)
