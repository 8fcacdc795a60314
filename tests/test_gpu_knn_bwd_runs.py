"""The backward gather of the KNN LUT (k_knn_bwd_tile, through ops.knn_lut_bwd) on shapes chosen for the seams of its tiling and of
the staging of a tile's query cells: a query grid that is no multiple of 16 with an odd number of tile columns, fewer workgroups than
the chip has CUs, tiles with far more than 256 (and 512) points, reaches beyond the largest staged halo, queries with the tie flag and
with the far flag, the flow_to_next gradient, 'iwd' weights and the L1 distance.

Reference: autograd through a brute-force K-nearest search in torch (never the library).  Bound: the relative L2 error of the
trajectory gradient that tests/test_gpu_parity.py holds the same quantity to against autograd through the oracle (1e-5)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIE_FLAG, FAR_FLAG = 0x40000000, 0x20000000
GRAD_REL_L2 = 1e-5          # tests/test_gpu_parity.py: dLUT -> trajectory gradient against autograd through the oracle


def _brute(traj, shape, sp, K, dist, scheme, want_next):
    """traj [B, 1 + nb, n, 2] on the device -> (lut [B, nb, hq, wq, 1, 2], next [B, nb - 1, hq, wq, 1, 2] or None), differentiable"""
    from oracle import focus_oracle as O
    grid, hq, wq = O.lut_grid_points(shape, sp)
    q = grid.to(traj.device)
    B, nb = traj.shape[0], traj.shape[1] - 1
    luts, nxts = [], []
    for b in range(B):
        lb, nbk = [], []
        for t in range(nb):
            pts = traj[b, 1 + t]
            diff = q[:, None, :] - pts.detach()[None, :, :]
            d = diff.abs().sum(-1) if dist == 'l1' else (diff ** 2).sum(-1)
            idx = torch.sort(d, dim=1, stable=True).indices[:, :K]
            f = (traj[b, 0] - pts)[idx]
            if scheme == 'iwd':
                w = 1.0 / (torch.gather(d, 1, idx) + 1e-9)
                w = (w / w.sum(1, keepdim=True)).detach()
                lb.append((f * w[..., None]).sum(1))
            else:
                lb.append(f.mean(1))
            if want_next and t < nb - 1:
                nbk.append((traj[b, 2 + t] - pts)[idx].mean(1))
        luts.append(torch.stack(lb))
        if want_next and nb > 1:
            nxts.append(torch.stack(nbk))
    lut = torch.stack(luts).reshape(B, nb, hq, wq, 1, 2)
    nxt = torch.stack(nxts).reshape(B, nb - 1, hq, wq, 1, 2) if (want_next and nb > 1) else None
    return lut, nxt


def _field(kind, B, H, W, g):
    if kind == 'lattice':            # no motion: the points stay on their lattice, K-th distances tie by the dozen
        return torch.zeros(B, 1, 2, H, W)
    if kind == 'smooth':             # coherent motion: regions contract and empty (far queries, reaches of many cells)
        c = torch.randn(B, 1, 2, H, W, generator=g) * 8.0
        return torch.nn.functional.avg_pool2d(c.reshape(B, 2, H, W), 31, 1, 15).reshape(B, 1, 2, H, W) * 20
    return torch.randn(B, 1, 2, H, W, generator=g) * float(kind)


# name: (image, superpixel, patch, B, bins, K, field, distance, scheme, flow_to_next, flag expected among the K-th indices or None)
CASES = {
    # 45 x 69 query cells: 3 x 5 tiles (odd tile columns, ragged last tile row and column), one launch of 15 workgroups
    'odd_columns_b1_one_bin': ((180, 276), 4, 4, 1, 1, 32, '3.0', 'l2', 'mean', False, None),
    # 2 x 3 tiles of 16 x 16 cells with 16 points per cell: ~4096 points per tile (many rounds of 256)
    'dense_tiles': ((248, 328), 8, 2, 1, 2, 32, '1.0', 'l2', 'mean', False, None),
    # one point per 8 x 8 pixels on 2-pixel cells: the K-th neighbour is ~13 cells away (beyond the largest staged halo of 9)
    'reach_beyond_staged_halo': ((128, 168), 2, 8, 1, 2, 32, '2.0', 'l2', 'mean', False, None),
    # halos around the largest staged one (6-10 cells) and both kinds of tile in one launch
    'large_halo_mixed': ((200, 264), 2, 4, 2, 2, 32, '6.0', 'l2', 'mean', False, None),
    'tie_flag': ((180, 276), 4, 4, 2, 3, 32, 'lattice', 'l2', 'mean', False, TIE_FLAG),
    'far_flag': ((480, 640), 4, 4, 1, 2, 32, 'smooth', 'l2', 'mean', False, FAR_FLAG),
    'flow_to_next': ((180, 276), 4, 4, 2, 3, 32, '3.0', 'l2', 'mean', True, None),
    'flow_to_next_iwd_l1': ((180, 276), 4, 4, 1, 3, 8, '3.0', 'l1', 'iwd', True, None),
    'iwd': ((180, 276), 4, 4, 2, 2, 32, '3.0', 'l2', 'iwd', False, None),
    'l1': ((180, 276), 4, 4, 2, 2, 32, '3.0', 'l1', 'mean', False, None),
    'tie_flag_l1_next': ((100, 148), 4, 4, 1, 3, 8, 'lattice', 'l1', 'mean', True, TIE_FLAG),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_knn_lut_bwd_against_bruteforce(name):
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    shape, sp, patch, B, nb, K, field, dist, scheme, want_next, flag = CASES[name]
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    coeff = _field(field, B, shape[0], shape[1], g)
    times = torch.cat((torch.tensor([0.37]), O.bin_mid_times(nb)))
    traj = O.trajectories_at(coeff, times, O.tile_mask(shape, patch), 1, 'polynomial')
    assert traj.shape[2] < 65536
    cfg = dict(image_shape=shape, num_tref=1, num_bins=nb, num_knn=K, smooth_weight=0.01, lut_superpixel_size=sp,
               focus_loss_norm='l1', dist_norm=dist, scale_iwe_by_dt=True, mask_image_border=True,
               polarity_aware_batching=True, interpolation_scheme=scheme,
               smooth_type='on_flow_to_next' if want_next else 'on_flow_to_tref')
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    trajd = traj.to(dev).contiguous()
    sh = ops.make_shape(L._cfg, B, 0, 0, traj.shape[2])
    ws = ops.alloc_workspace(sh, dev)
    lut, nxt, state, _ = ops.knn_lut_fwd(L._cfg, sh, trajd, ws)
    assert (nxt is not None) == want_next
    gl = torch.randn(lut.shape, generator=g).to(dev)
    gn = torch.randn(nxt.shape, generator=g).to(dev) if want_next else None
    with ops.KernelTimer() as kt:
        got = ops.knn_lut_bwd(sh, trajd, gl, gn, state, ws)
    assert any(k.startswith('k_knn_bwd_tile') for k in kt.summary()), set(kt.summary())
    if flag is not None:
        BQ = B * nb * lut.shape[2] * lut.shape[3]
        kth = state.view(torch.int32)[BQ:2 * BQ]
        assert int(((kth & flag) != 0).sum()) > 0, f'{name}: no query carries flag {flag:#x}'
    t2 = trajd.clone().requires_grad_(True)
    rl, rn = _brute(t2, shape, sp, K, dist, scheme, want_next)
    obj = (rl * gl).sum()
    if want_next:
        obj = obj + (rn * gn).sum()
    obj.backward()
    ref = t2.grad
    err = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    print(f'{name}: n {traj.shape[2]} rel-L2 of the trajectory gradient {err:.3e}')
    assert torch.isfinite(got).all()
    assert err < GRAD_REL_L2, (name, err)
    # the same call again: bit for bit
    again = ops.knn_lut_bwd(sh, trajd, gl, gn, state, ws)
    assert torch.equal(got, again)
