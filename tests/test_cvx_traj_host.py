"""The RAFT-spline output head on the host: the plain-torch mirror behind utils.trajectories_from_bezier(..., up_mask=...) and
utils.flows_from_bezier against the g13_cvx fixtures (tools/gen_golden_cvx.py: the unmodified reference's
BezierCurves(params).create_upsampled(mask).get_flow_from_reference(times) in fp32, a float64 evaluation of the same formula and the
measured distance between the two), and the unchanged behaviour without a mask.

Tolerance rule (shared with tests/test_gpu_cvx_traj.py): nothing fixed in advance -- for every tensor X the fixture holds
err_X = max |X_reference_fp32 - X_fp64|; the assertion is max |X - X_fp64| <= 4 * err_X, with the floor 2^-22 * max |X_fp64|.  The
margin 4 covers a different summation order and another exponential, each taken as worth about one more rounding of the 9- and
10-term sums.  `traj` gets half an ulp of the largest coordinate on top of the flows' tolerance for its one add."""
import numpy as np
import pytest
import torch

from conftest import load_golden

CASES = ['a', 'b', 'c', 'd', 'e']


def tol(g, name):
    return max(4.0 * float(g['err_' + name]), 2.0 ** -22 * float(np.abs(g[name + '64']).max()))


def tol_traj(g):
    return tol(g, 'flows') + float(np.spacing(np.float32(np.abs(g['traj64']).max()))) / 2


def inputs(g, device='cpu', grad=True):
    p = torch.from_numpy(g['params']).to(device).requires_grad_(grad)
    m = torch.from_numpy(g['mask']).to(device).requires_grad_(grad)
    h, w = p.shape[-2:]
    return p, m, torch.from_numpy(g['times']), int(g['tile']), (8 * h, 8 * w), float(g['scale'])


def maxdiff(t, ref64):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - ref64).max())


@pytest.mark.parametrize('case', CASES)
def test_mirror_matches_the_fixtures(case):
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_' + case)
    p, m, times, tile, shape, scale = inputs(g)
    traj, pos = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
    assert traj.shape == g['traj'].shape and traj.dtype == torch.float32
    assert torch.equal(pos, torch.nonzero(utils.get_optical_flow_tile_mask(shape, tile)))
    assert maxdiff(traj, g['traj64']) <= tol_traj(g)
    gp, gm = torch.autograd.grad(traj, [p, m], torch.from_numpy(g['g']))
    assert maxdiff(gp, g['grad_params64']) <= tol(g, 'grad_params')
    assert maxdiff(gm, g['grad_mask64']) <= tol(g, 'grad_mask')
    assert torch.isfinite(gm).all() and torch.isfinite(gp).all()
    flows = utils.flows_from_bezier(p.detach(), times, up_mask=m.detach(), scale=scale)
    assert flows.shape == (len(times),) + g['flows'].shape[1:]
    assert maxdiff(flows[g['flow_times']], g['flows64']) <= tol(g, 'flows')


@pytest.mark.parametrize('case', CASES)
def test_grad_mask_is_zero_off_the_tile_centre_channels(case):
    from motionpriorcmax_amd import utils
    g = load_golden('g13_cvx_' + case)
    p, m, times, tile, shape, scale = inputs(g)
    traj, pos = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
    (gm,) = torch.autograd.grad(traj, m, torch.from_numpy(g['g']))
    B, h, w = p.shape[0], p.shape[2], p.shape[3]
    touched = torch.zeros(9, 8, 8, h, w, dtype=torch.bool)
    touched[:, pos[:, 0] % 8, pos[:, 1] % 8, pos[:, 0] // 8, pos[:, 1] // 8] = True
    gm = gm.view(B, 9, 8, 8, h, w)
    assert float(gm[:, ~touched].abs().max()) == 0.0
    assert float(touched.float().mean()) == (min(8 // tile, 8) ** 2 / 64 if tile <= 8 else pos.shape[0] / (64 * h * w))
    # and the reference's own gradient vanishes there too
    assert float(np.abs(g['grad_mask'].reshape(B, 9, 8, 8, h, w)[:, ~touched.numpy()]).max()) == 0.0


def test_without_a_mask_nothing_changes():
    """up_mask=None: bitwise what the adapters returned before (the einsum / stack / add chain, spelled out here)."""
    from motionpriorcmax_amd import utils
    gen = torch.Generator().manual_seed(3)
    params = torch.randn(2, 8, 6, 8, generator=gen)
    times = torch.tensor([0.41, 0.1, 0.5, 0.9, 0.0, 1.0])
    for fn, bm in ((utils.trajectories_from_bezier, utils.bernstein_basis(times, 4)), (utils.trajectories_from_bspline, utils.bspline_basis(times, 5))):
        traj, pos = fn(params, times, 4, (24, 32), scale=8.0)
        traj2, pos2 = fn(params, times, 4, (24, 32), scale=8.0, up_mask=None)
        flow = torch.einsum('bcdhw,td->btchw', params.view(2, 2, 4, 6, 8), bm) * 8.0
        want = torch.stack((flow[:, :, 1], flow[:, :, 0]), dim=-1).reshape(2, 6, 48, 2) + pos.float()[None, None]
        assert torch.equal(traj, want) and torch.equal(traj2, want) and torch.equal(pos, pos2)
    flows = utils.flows_from_bezier(params, times, scale=8.0)
    assert torch.equal(flows, torch.einsum('bcdhw,td->tbchw', params.view(2, 2, 4, 6, 8), utils.bernstein_basis(times, 4)) * 8.0)


def test_a_mismatched_image_shape_raises():
    from motionpriorcmax_amd import utils
    params, mask, times = torch.zeros(1, 6, 2, 3), torch.zeros(1, 576, 2, 3), torch.tensor([0.5])
    for fn in (utils.trajectories_from_bezier, utils.trajectories_from_bspline):
        fn(params, times, 4, (16, 24), up_mask=mask)
        with pytest.raises(ValueError):
            fn(params, times, 4, (16, 32), up_mask=mask)
        with pytest.raises(ValueError):
            fn(params, times, 4, (8, 12), up_mask=mask)
        with pytest.raises(ValueError):
            fn(params, times, 4, (16, 24), up_mask=mask[:, :64])


def test_the_two_ends_of_the_curve():
    """t = 0 gives the tile centres themselves, t = 1 the last control point (reference base.py:102-106)."""
    from motionpriorcmax_amd import utils
    from motionpriorcmax_amd.utils.basis import _cvx_upsample
    g = load_golden('g13_cvx_a')
    p, m, times, tile, shape, scale = inputs(g, grad=False)
    d = p.shape[1] // 2
    traj, pos = utils.trajectories_from_bezier(p, times, tile, shape, scale=scale, up_mask=m)
    assert float(times[6]) == 0.0 and float(times[7]) == 1.0
    assert torch.equal(traj[:, 6], pos.float()[None].expand(p.shape[0], -1, -1))
    up = _cvx_upsample(p, m)[:, :, pos[:, 0], pos[:, 1]]
    want = pos.float()[None] + scale * torch.stack((up[:, 2 * d - 1], up[:, d - 1]), dim=-1)
    assert float((traj[:, 7] - want).abs().max()) <= tol_traj(g)
