"""The RAFT-spline output head on the device: utils.trajectories_from_bezier / _bspline(..., up_mask=...) -> ops.CvxCurveTrajFn and
utils.flows_from_bezier -> ops.cvx_flows (csrc/cvx_curves.hip: mpc_cvx_traj_fwd / _bwd, mpc_cvx_flow_fwd) against the g13_cvx
fixtures of the unmodified reference (tools/gen_golden_cvx.py), at the tolerance rule of tests/test_cvx_traj_host.py: for every
tensor max |X_gpu - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|) with err_X the reference's own fp32 error from the fixture;
`traj` gets half an ulp of its largest coordinate on top of the flows' tolerance for its one add.  Every figure is printed before
it is asserted (pytest -s shows them).

These bounds are one figure per tensor on five small inputs.  The kernels are held per element -- bit for bit on exact inputs, per
element under a counted rounding bound on weighted ones, at the fill chunks, tiles, basis sizes and template edges the fixtures do
not reach -- by tests/test_gpu_cvx_cases.py with tests/cvx_cases.py (cases, references, a restatement of the index arithmetic) and
tests/test_cvx_cases_host.py (census and mutants, on the CPU)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_cvx_traj_host import CASES, inputs, maxdiff, tol, tol_traj

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', 0)


def _check(label, got, bound):
    print(f'{label}: {got:.4g} (bound {bound:.4g})')
    assert got <= bound, (label, got, bound)


@pytest.mark.parametrize('case', CASES)
def test_goldens_through_the_public_functions(case):
    from motionpriorcmax_amd import ops, utils
    g = load_golden('g13_cvx_' + case)
    p, m, times, tile, shape, scale = inputs(g, _dev())
    with ops.KernelTimer() as kt:
        traj, pos = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
        gp, gm = torch.autograd.grad(traj, [p, m], torch.from_numpy(g['g']).to(_dev()))
        flows = utils.flows_from_bezier(p.detach(), times, up_mask=m.detach(), scale=scale)
    launches = {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}
    assert launches == {'k_cvx_traj_fwd': 1, 'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1, 'k_cvx_flow_fwd': 1}, launches
    assert traj.is_cuda and traj.dtype == torch.float32 and traj.is_contiguous() and traj.shape == g['traj'].shape
    assert torch.equal(pos, torch.nonzero(utils.get_optical_flow_tile_mask(shape, tile)))
    assert flows.shape == (len(times),) + g['flows'].shape[1:] and gp.shape == p.shape and gm.shape == m.shape
    assert torch.isfinite(traj).all() and torch.isfinite(gp).all() and torch.isfinite(gm).all() and torch.isfinite(flows).all()
    _check(f'{case} flows', maxdiff(flows[torch.from_numpy(g['flow_times']).to(_dev())], g['flows64']), tol(g, 'flows'))
    _check(f'{case} traj', maxdiff(traj, g['traj64']), tol_traj(g))
    _check(f'{case} grad_params', maxdiff(gp, g['grad_params64']), tol(g, 'grad_params'))
    _check(f'{case} grad_mask', maxdiff(gm, g['grad_mask64']), tol(g, 'grad_mask'))
    ref_zero = torch.from_numpy(g['grad_mask'] == 0)
    assert float(gm.cpu()[ref_zero].abs().max()) == 0.0


@pytest.mark.parametrize('case', ['a', 'e'])
def test_the_two_ends_of_the_curve(case):
    """The t = 0 row is the tile centres bitwise; the t = 1 row is pos + scale * up[:, d - 1] (reference base.py:102-106): the
    fixture's float64 flow at t = 1, within the flows' tolerance."""
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_' + case)
    p, m, times, tile, shape, scale = inputs(g, _dev(), grad=False)
    traj, pos = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
    assert float(times[6]) == 0.0 and float(times[7]) == 1.0 and int(g['flow_times'][2]) == 7
    assert torch.equal(traj[:, 6].cpu(), pos.float()[None].expand(p.shape[0], -1, -1))
    end = g['flows64'][2][:, :, pos[:, 0].numpy(), pos[:, 1].numpy()]                        # [B, (x, y), n]
    want = pos.numpy().astype(np.float64)[None] + np.stack((end[:, 1], end[:, 0]), axis=-1)
    _check(f'{case} t = 1 row', maxdiff(traj[:, 7], want), tol(g, 'flows'))


def _step(p0, m0, times, tile, shape, scale, go, mask_grad=True):
    from motionpriorcmax_amd import utils
    p = p0.clone().requires_grad_(True)
    m = m0.clone().requires_grad_(mask_grad)
    traj, _ = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
    grads = torch.autograd.grad(traj, [p, m] if mask_grad else [p], go)
    return (traj.detach(),) + tuple(grads)


def _case_e():
    g = load_golden('g13_cvx_e')
    p, m, times, tile, shape, scale = inputs(g, _dev(), grad=False)
    return p, m, times.to(_dev()), tile, shape, scale, torch.from_numpy(g['g']).to(_dev())


def test_two_runs_are_bitwise_equal():
    args = _case_e()
    a, b = _step(*args), _step(*args)
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(x.abs().max()) > 0 for x in a)


def test_capture_replays_bitwise_equal_to_eager():
    """Forward + backward captured into a torch.cuda.graph on one stream and replayed (the pattern of test_gpu_grid_traj.py: every leaf
    of the captured step is fresh)."""
    args = _case_e()
    eager = [t.clone() for t in _step(*args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture
        for _ in range(2):
            _step(*args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(*args)
    graph.replay()
    torch.cuda.synchronize()
    assert len(static) == len(eager) == 3
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


def test_no_host_synchronisation_in_either_direction():
    from motionpriorcmax_amd import utils
    args = _case_e()
    p, m, times, tile, shape, scale, go = args
    _step(*args)                                                 # warm-up: library load, cached basis and tile positions
    utils.flows_from_bezier(p, times, up_mask=m, scale=scale)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _step(*args)
        flows = utils.flows_from_bezier(p, times, up_mask=m, scale=scale)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out[1].shape == p.shape and out[2].shape == m.shape and flows.shape[0] == times.shape[0]


def test_bspline_basis_with_a_mask_matches_the_mirror():
    """Case-a inputs, the cubic B-spline basis: the kernels against the plain-torch mirror evaluated in float64, at the rule of the
    goldens with the mirror's own fp32 error in the place of the reference's."""
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_a')
    p, m, times, tile, shape, scale = inputs(g, _dev())
    go = torch.from_numpy(g['g'])

    def run(pp, mm, gg):
        traj, _ = utils.trajectories_from_bspline(pp, times, tile, shape, scale=scale, up_mask=mm)
        return (traj.detach(),) + torch.autograd.grad(traj, [pp, mm], gg)

    p32, m32 = (t.detach().cpu().requires_grad_(True) for t in (p, m))
    p64, m64 = (t.detach().cpu().double().requires_grad_(True) for t in (p, m))
    mir32, mir64, got = run(p32, m32, go), run(p64, m64, go.double()), run(p, m, go.to(_dev()))
    assert mir64[0].dtype == torch.float64
    for name, a32, a64, a in zip(('traj', 'grad_params', 'grad_mask'), mir32, mir64, got):
        a64 = a64.numpy()
        bound = max(4.0 * maxdiff(a32, a64), 2.0 ** -22 * float(np.abs(a64).max()))
        if name == 'traj':
            bound += float(np.spacing(np.float32(np.abs(a64).max()))) / 2
        _check(f'bspline {name}', maxdiff(a, a64), bound)


def test_only_the_requested_gradients_are_produced():
    gen = torch.Generator().manual_seed(21)
    B, d, h, w, tile = 2, 10, 12, 16, 4
    p = (torch.randn(B, 2 * d, h, w, generator=gen) * 0.5).to(_dev())
    m = (torch.randn(B, 576, h, w, generator=gen) * 2.0).to(_dev())
    times = torch.tensor([0.41, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0, 1.0]).to(_dev())
    go = torch.randn(B, 8, (8 * h // tile) * (8 * w // tile), 2, generator=gen).to(_dev())
    args = (p, m, times, tile, (8 * h, 8 * w), 1.0, go)
    both = _step(*args)
    _step(*args, mask_grad=False)                                # warm-up of this path
    from motionpriorcmax_amd import utils
    pp = p.clone().requires_grad_(True)
    traj, _ = utils.trajectories_from_bezier(pp, times, tile, (8 * h, 8 * w), up_mask=m)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    (gp,) = torch.autograd.grad(traj, pp, go)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f'backward without a mask gradient: peak memory grew by {grew} B; a grad_mask is {m.numel() * 4} B')
    assert grew < m.numel() * 4
    assert torch.equal(gp, both[1])


def test_abi_refuses_bad_arguments_without_launching():
    from motionpriorcmax_amd import ops, _lib as C
    x = torch.zeros(1 << 16, device=_dev())
    v = ctypes.c_void_p(x.data_ptr())
    L = C.lib()
    with ops.KernelTimer() as kt:
        # null pointers
        assert L.mpc_cvx_traj_fwd(None, v, v, 1.0, v, 1, 3, 2, 2, 2, 4, None) == C.E_NULL
        assert b'null' in L.mpc_last_error_string()
        assert L.mpc_cvx_traj_fwd(v, None, v, 1.0, v, 1, 3, 2, 2, 2, 4, None) == C.E_NULL
        assert L.mpc_cvx_traj_fwd(v, v, None, 1.0, v, 1, 3, 2, 2, 2, 4, None) == C.E_NULL
        assert L.mpc_cvx_traj_fwd(v, v, v, 1.0, None, 1, 3, 2, 2, 2, 4, None) == C.E_NULL
        assert L.mpc_cvx_flow_fwd(v, v, v, 1.0, None, 1, 3, 2, 2, 2, None) == C.E_NULL
        assert L.mpc_cvx_traj_bwd(None, v, v, v, 1.0, v, v, 1, 3, 2, 2, 2, 4, v, None) == C.E_NULL
        assert L.mpc_cvx_traj_bwd(v, v, v, v, 1.0, v, v, 1, 3, 2, 2, 2, 4, None, None) == C.E_NULL       # grad_params without a workspace
        # d = 0, d = 17, tile = 0, negative h
        for fn, args in ((L.mpc_cvx_traj_fwd, lambda d, h, tile: (v, v, v, 1.0, v, 1, d, 2, h, 2, tile, None)),
                         (L.mpc_cvx_traj_bwd, lambda d, h, tile: (v, v, v, v, 1.0, v, v, 1, d, 2, h, 2, tile, v, None)),
                         (L.mpc_cvx_flow_fwd, lambda d, h, tile: (v, v, v, 1.0, v, 1, d, 2, h, 2, None)),
                         (L.mpc_cvx_traj_bwd_workspace_bytes, lambda d, h, tile: (1, d, 2, h, 2, tile))):
            assert fn(*args(0, 2, 4)) == C.E_SHAPE
            assert fn(*args(17, 2, 4)) == C.E_UNSUPPORTED
            assert b'control points' in L.mpc_last_error_string()
            assert fn(*args(3, -1, 4)) == C.E_SHAPE
            if fn is not L.mpc_cvx_flow_fwd:
                assert fn(*args(3, 2, 0)) == C.E_SHAPE
        # a basis matrix beyond the LDS slice; B = 0 launches nothing
        assert L.mpc_cvx_traj_fwd(v, v, v, 1.0, v, 1, 16, 769, 2, 2, 4, None) == C.E_UNSUPPORTED
        assert L.mpc_cvx_traj_fwd(v, v, v, 1.0, v, 0, 3, 2, 2, 2, 4, None) == 0
        assert L.mpc_cvx_traj_bwd(v, v, v, v, 1.0, v, v, 0, 3, 2, 2, 2, 4, v, None) == 0
        assert L.mpc_cvx_flow_fwd(v, v, v, 1.0, v, 0, 3, 2, 2, 2, None) == 0
    assert kt.summary() == {}
    assert L.mpc_cvx_traj_bwd_workspace_bytes(2, 10, 8, 12, 16, 4) >= 2 * 24 * 32 * 29 * 4


def test_the_loss_accepts_the_result():
    """FocusLoss.calc on a 32 x 48 image with trajectories from the node; backward() leaves finite, non-zero gradients in params and
    up_mask.  (No loss value is compared: a 1e-6 trajectory difference can flip a neighbour set.)"""
    from motionpriorcmax_amd import LossFactory, utils
    from motionpriorcmax_amd.utils.synth import synth_events
    dev = _dev()
    nb = 5
    L = LossFactory.get_loss_calculator('FOCUS', dict(image_shape=(32, 48), num_tref=1, num_bins=nb, num_knn=4, smooth_weight=0.003,
                                                      lut_superpixel_size=4, focus_loss_norm='l1', dist_norm='l2',
                                                      scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
                                                      interpolation_scheme='mean', smooth_type='on_flow_to_tref'))
    ev, num_pos = synth_events(2, 3000, (32, 48), nb, seed=2, pad_frac=0.02)
    gen = torch.Generator().manual_seed(5)
    p = (torch.randn(2, 6, 4, 6, generator=gen) * 0.25).to(dev).requires_grad_(True)
    m = (torch.randn(2, 576, 4, 6, generator=gen) * 2.0).to(dev).requires_grad_(True)
    times = L.get_reconstruction_times(dev)
    traj, pos = utils.trajectories_from_bezier(p, times, 4, (32, 48), up_mask=m)
    assert traj.shape == (2, 1 + nb, 8 * 12, 2)
    loss, _, _ = L.calc(traj, times, {'events': ev.to(dev), 'num_pos_events': num_pos})
    loss.backward()
    assert torch.isfinite(loss)
    for t in (p, m):
        assert t.grad is not None and torch.isfinite(t.grad).all() and float(t.grad.abs().max()) > 0
