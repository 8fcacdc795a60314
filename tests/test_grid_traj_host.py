"""utils.trajectories_from_grid / flow_from_grid on the host (the plain-torch mirror CPU tensors take): the reference's
TrajectoryNet.calculate_trajectories_at_t (trajectory_net.py:101-119) against the goldens, the tile count and order against
torch.nonzero of the tile mask, and calculate_flow's composition (:121-140)."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN_CASES, load_golden


def _net(g):
    net = nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(),
                        nn.Linear(64, int(g['num_basis'])))
    net.load_state_dict({k: torch.from_numpy(g['net_' + k.replace('.', '_')]) for k in net.state_dict()})
    return net


@pytest.mark.parametrize('name', GOLDEN_CASES + ['g11_learned_basis'])
def test_cpu_trajectories_from_grid_match_goldens(name):
    from motionpriorcmax_amd import utils
    from oracle import focus_oracle as O
    g = load_golden(name)
    k, patch = int(g['num_basis']), int(g['patch'])
    bt = 'learned' if name == 'g11_learned_basis' else str(g['basis_type'])
    net = _net(g) if bt == 'learned' else None
    cg = torch.from_numpy(g['coeff_grid'])
    times = torch.from_numpy(g['times'])
    traj, pos = utils.trajectories_from_grid(cg, times, k, bt, patch, basis_network=net)
    assert traj.shape == g['trajectories'].shape and traj.is_contiguous()
    np.testing.assert_allclose(traj.detach().numpy(), g['trajectories'], rtol=0, atol=1e-5)
    mask = utils.get_optical_flow_tile_mask(g['cfg']['image_shape'], patch)
    assert torch.equal(pos, torch.nonzero(mask))
    if bt != 'learned':
        ref = O.trajectories_at(cg, times, O.tile_mask(g['cfg']['image_shape'], patch), k, bt)
        np.testing.assert_allclose(traj.numpy(), ref.numpy(), rtol=0, atol=1e-6)
    # a 4-dim grid is S = 1 (trajectory_net.py:113-114)
    traj4, _ = utils.trajectories_from_grid(cg[:, 0], times, k, bt, patch, basis_network=net)
    assert torch.equal(traj4, traj)


@pytest.mark.parametrize('tile', [1, 3, 4, 5, 8])
@pytest.mark.parametrize('hw', [(48, 64), (50, 70), (13, 9), (3, 2)])
def test_tile_count_and_order_match_the_tile_mask(tile, hw):
    from motionpriorcmax_amd import utils
    from motionpriorcmax_amd.utils.grid_traj import grid_tile_counts
    ref = torch.nonzero(utils.get_optical_flow_tile_mask(hw, tile))
    hq, wq = grid_tile_counts(hw[0], hw[1], tile)
    assert hq * wq == ref.shape[0]
    s = tile // 2
    assert hq == len(range(s, hw[0], tile)) and wq == len(range(s, hw[1], tile))
    g = torch.Generator().manual_seed(tile)
    cg = torch.randn(2, 2, 4, *hw, generator=g)
    traj, pos = utils.trajectories_from_grid(cg, torch.tensor([0.0, 0.3, 1.0]), 2, 'polynomial', tile)
    assert pos.dtype == torch.int64 and torch.equal(pos, ref)
    assert traj.shape == (2, 3, ref.shape[0], 2)
    # t = 0 is the anchor: every trajectory starts at its tile centre
    assert torch.equal(traj[:, 0], ref.float()[None].expand(2, -1, -1))


def test_tile_count_differs_from_ceil_division_where_it_must():
    from motionpriorcmax_amd.utils.grid_traj import grid_tile_counts
    assert grid_tile_counts(50, 70, 8) == (6, 9)           # ceil(50 / 8) = 7, ceil(70 / 8) = 9
    assert grid_tile_counts(3, 2, 8) == (0, 0)


def test_cpu_mirror_gradient_and_errors():
    from motionpriorcmax_amd import utils
    from oracle import focus_oracle as O
    g = torch.Generator().manual_seed(3)
    c = torch.randn(1, 2, 6, 24, 20, generator=g)
    cg = c.clone().requires_grad_(True)
    times = torch.tensor([0.41, 0.1, 0.5, 0.9])
    traj, _ = utils.trajectories_from_grid(cg, times, 3, 'dct', 4, anchor_time=0.25)
    co = c.clone().requires_grad_(True)
    ref = O.trajectories_at(co, times, O.tile_mask((24, 20), 4), 3, 'dct', anchor_time=0.25)
    np.testing.assert_allclose(traj.detach().numpy(), ref.detach().numpy(), rtol=0, atol=1e-6)
    go = torch.randn(traj.shape, generator=g)
    traj.backward(go)
    ref.backward(go)
    np.testing.assert_allclose(cg.grad.numpy(), co.grad.numpy(), rtol=0, atol=1e-5)
    m = utils.get_optical_flow_tile_mask((24, 20), 4)
    assert cg.grad[..., ~m].abs().max() == 0
    with pytest.raises(ValueError):
        utils.trajectories_from_grid(c, times, 3, 'bezier', 4)
    with pytest.raises(ValueError):
        utils.trajectories_from_grid(c, times, 2, 'polynomial', 4)


def test_cpu_flow_from_grid_is_calculate_flow(monkeypatch):
    """calculate_flow (trajectory_net.py:121-140): compute_basis at t_end minus at the anchor 0, at the tile centres, spread to a dense
    flow.  The dense step is a GPU operator in this package; on the host the oracle's transcription of the reference's
    dense_flow_from_traj (list_to_grid + antialiased bicubic resize) stands in for it."""
    from motionpriorcmax_amd import utils
    from motionpriorcmax_amd.utils import flow as flow_mod
    from oracle import flow_oracle as FO
    monkeypatch.setattr(flow_mod, 'dense_flow_from_traj', FO.dense_flow_from_traj)
    g = load_golden('g5a_dct3_l2')
    k, patch, shape = int(g['num_basis']), int(g['patch']), g['cfg']['image_shape']
    cg = torch.from_numpy(g['coeff_grid'])
    for t_end in (1.0, 0.5):
        got = utils.flow_from_grid(cg, k, str(g['basis_type']), patch, shape, t_end=t_end)
        coeffs, pos, _ = utils.coeffs_grid_to_list(cg, utils.get_optical_flow_tile_mask(shape, patch), k)
        flow = utils.compute_basis(coeffs, torch.tensor([t_end]), k, 'dct') - utils.compute_basis(coeffs, torch.tensor([0.0]), k, 'dct')
        want, _ = FO.dense_flow_from_traj(flow[..., 0, :], pos, patch, shape)
        assert got.shape == (cg.shape[0], 2) + tuple(shape)
        assert np.array_equal(np.asarray(got), want)
