"""The coefficient grid -> trajectories node on the device (utils.trajectories_from_grid -> ops.GridTrajFn, csrc/grid_traj.hip:
mpc_grid_traj_fwd / _bwd) against the reference's chain (TrajectoryNet.calculate_trajectories_at_t, trajectory_net.py:101-119:
coeffs_grid_to_list -> compute_basis at the times minus at the anchor -> + pixel positions) on the same device inputs: forward, the
adjoint, the reference's goldens end to end through `calc`, no host synchronisation, launch counts, determinism, the DSEC batch size
and the ABI's argument errors."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', 0)


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def _net(g, device):
    net = nn.Sequential(nn.Linear(1, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(), nn.Linear(64, 64), nn.LeakyReLU(),
                        nn.Linear(64, int(g['num_basis'])))
    net.load_state_dict({k: torch.from_numpy(g['net_' + k.replace('.', '_')]) for k in net.state_dict()})
    return net.to(device)


def _mirror(cg, times, k, bt, tile, add_offsets=True, net=None, anchor=0.0):
    """The reference's chain in plain torch on the grid's device (the glue the node replaces)."""
    from motionpriorcmax_amd import utils
    if cg.dim() == 4:
        cg = cg[:, None]
    mask = utils.get_optical_flow_tile_mask(tuple(cg.shape[-2:]), tile).to(cg.device)
    coeffs, pos, _ = utils.coeffs_grid_to_list(cg, mask, k)
    a = torch.full((1,), anchor, device=cg.device, dtype=coeffs.dtype)
    traj = utils.compute_basis(coeffs, times, k, bt, net) - utils.compute_basis(coeffs, a, k, bt, net)
    if add_offsets:
        traj = traj + pos[None, :, None, :]
    return traj.permute(0, 2, 1, 3).contiguous()


def _poisoned_block(shape, dev):
    """Empty the allocator's cache, allocate a NaN-filled fp32 tensor of `shape`, free it: the next allocation of that size on this
    stream gets the same block (the allocator's free lists are as they were before the NaN tensor).  Returns its address."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full(shape, float('nan'), device=dev)
    ptr = poison.data_ptr()
    del poison
    return ptr


_LOSS = []


def _times(dev, nb=15):
    """FocusLoss.get_reconstruction_times: t_ref drawn with torch.rand ON THE DEVICE, then the bin mid-times."""
    if not _LOSS:
        _LOSS.append(_loss(nb))
    return _LOSS[0].get_reconstruction_times(dev)


def _loss(nb):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', dict(image_shape=(48, 64), num_tref=1, num_bins=nb, num_knn=4, smooth_weight=0.0,
                                                      lut_superpixel_size=4, focus_loss_norm='l1', dist_norm='l2',
                                                      scale_iwe_by_dt=False, mask_image_border=False, polarity_aware_batching=False,
                                                      interpolation_scheme='mean', smooth_type='on_flow_to_tref'))


FWD_CASES = [  # (basis, k, S, tile, B, (H, W), anchor)
    ('polynomial', 1, 1, 4, 1, (48, 64), 0.0),
    ('polynomial', 3, 3, 4, 3, (50, 70), 0.25),
    ('polynomial', 8, 1, 3, 1, (31, 29), 0.0),
    ('polynomial', 16, 3, 8, 3, (50, 70), 0.25),
    ('dct', 1, 3, 1, 1, (13, 300), 0.0),             # two workgroup chunks per row of the backward (tile 1, W > 256)
    ('dct', 3, 1, 4, 3, (48, 64), 0.25),
    ('dct', 8, 3, 8, 1, (50, 70), 0.0),
    ('dct', 16, 1, 3, 3, (22, 23), 0.25),
]


@pytest.mark.parametrize('bt,k,S,tile,B,hw,anchor', FWD_CASES)
def test_forward_matches_the_reference_chain(bt, k, S, tile, B, hw, anchor):
    from motionpriorcmax_amd import utils
    from oracle import focus_oracle as O
    dev = _dev()
    g = torch.Generator().manual_seed(k * 100 + tile)
    cg = (torch.randn(B, S, 2 * k, *hw, generator=g) * 2.0).to(dev)
    times = _times(dev)
    mask = O.tile_mask(hw, tile).to(dev)
    ref = O.trajectories_at(cg, times, mask, k, bt, add_offsets=False, anchor_time=anchor)
    disp, pos = utils.trajectories_from_grid(cg, times, k, bt, tile, add_offsets=False, anchor_time=anchor)
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous() and disp.shape == ref.shape
    assert pos.is_cuda and pos.dtype == torch.int64 and torch.equal(pos.cpu(), torch.nonzero(O.tile_mask(hw, tile)))
    tol = 2e-6 * float(ref.abs().max()) + 1e-6
    assert float((disp - ref).abs().max()) <= tol
    traj, _ = utils.trajectories_from_grid(cg, times, k, bt, tile, add_offsets=True, anchor_time=anchor)
    want = disp + pos.float()[None, None]
    ulp = float(torch.finfo(torch.float32).eps) * float(pos.max().clamp(min=1))
    assert float((traj - want).abs().max()) <= ulp
    # a 4-dim grid is S = 1
    if S == 1:
        t4, _ = utils.trajectories_from_grid(cg[:, 0], times, k, bt, tile, add_offsets=True, anchor_time=anchor)
        assert torch.equal(t4, traj)


@pytest.mark.parametrize('bt,k,S,tile,B,hw,anchor', FWD_CASES + [('learned', 3, 2, 4, 2, (50, 70), 0.25), ('learned', 3, 1, 4, 1, (48, 64), 0.0)])
def test_backward_matches_the_reference_chain(bt, k, S, tile, B, hw, anchor):
    from motionpriorcmax_amd import utils
    dev = _dev()
    g = torch.Generator().manual_seed(k * 10 + S)
    c = torch.randn(B, S, 2 * k, *hw, generator=g) * 2.0
    times = _times(dev)
    net = None
    if bt == 'learned':
        torch.manual_seed(4)
        net = nn.Sequential(nn.Linear(1, 16), nn.LeakyReLU(), nn.Linear(16, k)).to(dev)
    cm = c.to(dev).requires_grad_(True)
    ref = _mirror(cm, times, k, bt, tile, net=net, anchor=anchor)
    go = torch.randn(ref.shape, generator=g).to(dev)
    mirror_net_grads = None
    if net is not None:
        mirror_net_grads = torch.autograd.grad(ref, [cm] + list(net.parameters()), go)
        gm = mirror_net_grads[0]
    else:
        (gm,) = torch.autograd.grad(ref, cm, go)
    cf = c.to(dev).requires_grad_(True)
    traj, _ = utils.trajectories_from_grid(cf, times, k, bt, tile, basis_network=net, anchor_time=anchor)
    # every element must be written by the kernel (torch.empty is all that stands behind the gradient): with the cache emptied, a
    # NaN-filled block of the gradient's size freed just before the backward is the block the gradient gets -- asserted below
    gptr = _poisoned_block((B, S, 2 * k) + hw, dev)
    if net is not None:
        fused = torch.autograd.grad(traj, [cf] + list(net.parameters()), go)
        gf = fused[0]
    else:
        (gf,) = torch.autograd.grad(traj, cf, go)
    assert gf.data_ptr() == gptr and not torch.isnan(gf).any()
    mask = utils.get_optical_flow_tile_mask(hw, tile).to(dev)
    assert _rel_l2(gf[..., mask], gm[..., mask]) <= 1e-5
    assert float(gf[..., ~mask].abs().max()) == 0.0 if (~mask).any() else True
    for s in range(1, S):
        assert torch.equal(gf[:, s], gf[:, 0])
    if net is not None:
        # (the last bias cancels in net(t) - net(anchor): its gradient is rounding noise, hence a floor from the largest)
        top = max(float(b.norm()) for b in mirror_net_grads[1:])
        for a, b in zip(fused[1:], mirror_net_grads[1:]):
            assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-5 * top


def test_learned_dphi_gradient_matches_the_mirror():
    """grad_dphi of the node (the partial sums of k_grid_traj_bwd + k_grid_dphi_sum) against autograd through the mirror."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    B, S, k, H, W, tile = 3, 2, 5, 50, 70, 4
    c = (torch.randn(B, S, 2 * k, H, W, generator=g)).to(dev)
    times = _times(dev)
    d0 = torch.randn(times.shape[0], k, generator=g).to(dev)
    dph = d0.clone().requires_grad_(True)
    cf = c.clone().requires_grad_(True)
    traj = ops.GridTrajFn.apply(cf, times, dph, C.BASIS_MATRIX, 0.0, True, tile)
    go = torch.randn(traj.shape, generator=g).to(dev)
    gc, gd = torch.autograd.grad(traj, [cf, dph], go)
    # mirror: the same product in plain torch
    from motionpriorcmax_amd import utils
    mask = utils.get_optical_flow_tile_mask((H, W), tile).to(dev)
    cm = c.clone().requires_grad_(True)
    dm = d0.clone().requires_grad_(True)
    coeffs, pos, _ = utils.coeffs_grid_to_list(cm, mask, k)
    cs = coeffs.sum(1)                                                        # [B, 2, n, k]
    disp = torch.einsum('tj,bdnj->btnd', dm, cs)
    ref = disp + pos[None, None]
    gcm, gdm = torch.autograd.grad(ref, [cm, dm], go)
    assert _rel_l2(traj, ref) <= 1e-6
    assert _rel_l2(gc[..., mask], gcm[..., mask]) <= 1e-5
    assert _rel_l2(gd, gdm) <= 1e-5


@pytest.mark.parametrize('name', ['g1_allflags', 'g5a_dct3_l2', 'g5b_poly3', 'g11_learned_basis'])
def test_training_step_from_the_grid_matches_reference_goldens(name):
    from motionpriorcmax_amd import utils, LossFactory
    g = load_golden(name)
    dev = _dev()
    cfg = g['cfg']
    k, patch = int(g['num_basis']), int(g['patch'])
    bt = 'learned' if name == 'g11_learned_basis' else str(g['basis_type'])
    net = _net(g, dev) if bt == 'learned' else None
    cg = torch.from_numpy(g['coeff_grid']).to(dev).requires_grad_(True)
    times = torch.from_numpy(g['times']).to(dev)
    traj, pos = utils.trajectories_from_grid(cg, times, k, bt, patch, basis_network=net)
    np.testing.assert_allclose(traj.detach().cpu().numpy(), g['trajectories'], rtol=0, atol=1e-5)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    batch = {'events': torch.from_numpy(g['events']).to(dev)}
    if cfg['polarity_aware_batching']:
        batch['num_pos_events'] = int(g['num_pos'])
    loss, _, _ = L.calc(traj, times, batch)
    loss.backward()
    assert abs(loss.item() - float(g['loss'])) <= 1e-5 * abs(float(g['loss']))
    gc = cg.grad.cpu().numpy()
    m = utils.get_optical_flow_tile_mask(cfg['image_shape'], patch).numpy()
    ref = g['grad_coeff_grid_at_tiles']
    assert np.abs(gc[..., ~m]).max() == float(g.get('grad_coeff_grid_off_tiles_abs_max', 0.0)) == 0.0
    d = gc[..., m] - ref
    rel = np.linalg.norm(d) / np.linalg.norm(ref)
    bad = np.abs(d) > 2e-5 * np.abs(ref).max() + 1e-4 * np.abs(ref)
    assert rel < (1e-4 if cfg['focus_loss_norm'] == 'l2' else 1e-3), rel
    assert bad.mean() <= 1e-3, (bad.mean(), rel)
    from grad_accounting import end_to_end_accounting
    iwes = torch.from_numpy(g['iwes']) if 'iwes' in g else None
    end_to_end_accounting(cfg, torch.from_numpy(g['events']), int(g['num_pos']), torch.from_numpy(g['trajectories']), gc[..., m], ref,
                          blurred=iwes, t_ref=torch.from_numpy(g['times'])[:cfg['num_tref']], grid=True, label=f'{name} grid gradient')
    if net is not None:
        top = max(np.linalg.norm(g[kk]) for kk in g if kk.startswith('grad_net_'))
        for pname, prm in net.named_parameters():
            r = g['grad_net_' + pname.replace('.', '_')]
            assert np.linalg.norm(prm.grad.cpu().numpy() - r) <= 1e-3 * np.linalg.norm(r) + 1e-4 * top, pname


def _c3_grid(dev, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(14, 1, 6, 480, 640, generator=g).to(dev)


def test_no_host_synchronisation_in_either_direction():
    """At the DSEC batch shape with device-drawn times: the node raises nothing under sync debug mode 'error'; the plain-torch chain
    (its mask gather runs nonzero) must raise -- the test tells the two apart."""
    from motionpriorcmax_amd import utils
    dev = _dev()
    c = _c3_grid(dev)
    gout = torch.randn(14, 16, 120 * 160, 2, device=dev)
    # warm-up outside the checked region (library load, cached tile positions, LDS set-up)
    t0 = _times(dev)
    cw = c.clone().requires_grad_(True)
    tw, _ = utils.trajectories_from_grid(cw, t0, 3, 'polynomial', 4)
    torch.autograd.backward(tw, gout)
    torch.cuda.synchronize()

    def fused():
        cg = c.clone().requires_grad_(True)
        times = _times(dev)
        traj, _ = utils.trajectories_from_grid(cg, times, 3, 'polynomial', 4)
        torch.autograd.backward(traj, gout)
        return cg

    def glue():
        cg = c.clone().requires_grad_(True)
        times = _times(dev)
        traj = _mirror(cg, times, 3, 'polynomial', 4)
        torch.autograd.backward(traj, gout)

    torch.cuda.set_sync_debug_mode('error')
    try:
        cg = fused()
        with pytest.raises(RuntimeError):
            glue()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert cg.grad is not None and cg.grad.shape == c.shape


@pytest.mark.parametrize('bt', ['polynomial', 'dct', 'learned'])
def test_launch_counts(bt):
    from motionpriorcmax_amd import ops, utils
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    cg = torch.randn(2, 1, 6, 48, 64, generator=g).to(dev).requires_grad_(True)
    net = nn.Sequential(nn.Linear(1, 8), nn.LeakyReLU(), nn.Linear(8, 3)).to(dev) if bt == 'learned' else None
    times = _times(dev)
    with ops.KernelTimer() as kf:
        traj, _ = utils.trajectories_from_grid(cg, times, 3, bt, 4, basis_network=net)
    go = torch.randn(traj.shape, device=dev)
    with ops.KernelTimer() as kb:
        traj.backward(go)
    nf = sum(r['launches'] for r in kf.summary().values())
    nbw = sum(r['launches'] for r in kb.summary().values())
    assert nf == 1, kf.summary()
    if bt == 'learned':
        assert 1 <= nbw <= 2, kb.summary()
        assert all(p.grad is not None for p in net.parameters())
    else:
        assert nbw == 1, kb.summary()


@pytest.mark.parametrize('bt', ['polynomial', 'learned'])
def test_deterministic(bt):
    """Two runs of the node, bitwise: trajectories, the grid gradient and (learned) grad_dphi taken directly from a leaf dphi."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    c = torch.randn(3, 2, 6, 50, 70, generator=g).to(dev)
    times = _times(dev)
    d0 = torch.randn(times.shape[0], 3, generator=g).to(dev)
    outs = []
    for _ in range(2):
        cg = c.clone().requires_grad_(True)
        if bt == 'learned':
            dph = d0.clone().requires_grad_(True)
            traj = ops.GridTrajFn.apply(cg, times, dph, C.BASIS_MATRIX, 0.0, True, 4)
            w = torch.linspace(-1, 1, traj.numel(), device=dev).view_as(traj)
            gc, gd = torch.autograd.grad(traj, [cg, dph], w)
        else:
            traj = ops.GridTrajFn.apply(cg, times, None, C.BASIS_POLY, 0.0, True, 4)
            w = torch.linspace(-1, 1, traj.numel(), device=dev).view_as(traj)
            (gc,) = torch.autograd.grad(traj, cg, w)
            gd = torch.zeros(1, device=dev)
        outs.append((traj.detach().clone(), gc, gd))
    (a, ga, da), (b, gb, db) = outs
    assert torch.equal(a, b) and torch.equal(ga, gb) and torch.equal(da, db)
    if bt == 'learned':
        assert float(da.abs().max()) > 0


def test_learned_gradient_with_an_empty_batch_is_zero():
    """B = 0: no grid element, but grad_dphi (torch.empty behind it) is still written -- zeros."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    times = _times(dev)
    cg = torch.zeros(0, 1, 6, 48, 64, device=dev, requires_grad=True)
    dph = torch.randn(times.shape[0], 3, device=dev).requires_grad_(True)
    traj = ops.GridTrajFn.apply(cg, times, dph, C.BASIS_MATRIX, 0.0, True, 4)
    assert traj.shape == (0, times.shape[0], 12 * 16, 2)
    gptr = _poisoned_block((times.shape[0], 3), dev)
    gc, gd = torch.autograd.grad(traj, [cg, dph], torch.zeros_like(traj))
    assert gc.shape == cg.shape
    assert gd.data_ptr() == gptr and torch.equal(gd, torch.zeros_like(gd))


def test_basis_beyond_the_lds_slice_takes_the_mirror():
    """n_t * k > 4096 (k = 16, 300 times) is beyond the kernels' LDS slice of the basis: the plain-torch mirror serves it."""
    from motionpriorcmax_amd import ops, utils
    dev = _dev()
    g = torch.Generator().manual_seed(12)
    c = torch.randn(1, 1, 32, 24, 32, generator=g).to(dev)
    times = torch.rand(300, generator=g).to(dev)
    with ops.KernelTimer() as kt:
        traj, _ = utils.trajectories_from_grid(c, times, 16, 'polynomial', 4)
    assert kt.summary() == {}
    assert torch.equal(traj, _mirror(c, times, 16, 'polynomial', 4))
    small, _ = utils.trajectories_from_grid(c, times[:256], 16, 'polynomial', 4)      # 4096 values: the kernels
    assert float((small - traj[:, :256]).abs().max()) <= 2e-6 * float(traj.abs().max()) + 1e-6


@pytest.mark.parametrize('bt', ['polynomial', 'learned'])
def test_capture_replays_bitwise_equal_to_eager(bt):
    """The node's forward + backward captured into a torch.cuda.graph on one stream and replayed: bitwise the eager results.
    Every leaf of the captured step is fresh: an autograd graph kept alive from an eager run on the default stream would leave its
    AccumulateGrad nodes on that stream, and the backward would reach from the capture stream into the legacy default stream
    (torch warns of exactly this: 'break CUDA graph capture if the AccumulateGrad node's stream is the default stream')."""
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    c = torch.randn(2, 1, 6, 96, 128, generator=g).to(dev)
    times = _times(dev)
    d0 = torch.randn(times.shape[0], 3, generator=g).to(dev)
    go = torch.randn(2, times.shape[0], 24 * 32, 2, generator=g).to(dev)
    basis = C.BASIS_MATRIX if bt == 'learned' else C.BASIS_POLY

    def step():
        cg = c.clone().requires_grad_(True)
        dph = d0.clone().requires_grad_(True) if bt == 'learned' else None
        traj = ops.GridTrajFn.apply(cg, times, dph, basis, 0.0, True, 4)
        grads = torch.autograd.grad(traj, [cg] + ([dph] if dph is not None else []), go)
        return (traj.detach(),) + tuple(grads)

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    assert len(static) == len(eager)
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


def test_dsec_size_step_from_the_grid_matches_the_glue_step():
    """[14, 1, 6, 480, 640], polynomial k = 3, tile 4, focus_loss_norm 'l2' (smooth objective): the whole training step from the grid
    through the node against the same step through the plain-torch chain."""
    import bench
    from motionpriorcmax_amd import utils, LossFactory
    from motionpriorcmax_amd.utils.synth import synth_events
    dev = _dev()
    wl = bench.WORKLOADS['C3']
    cfg = dict(bench.loss_config(wl), focus_loss_norm='l2')
    ev, num_pos = synth_events(14, wl['M'], (480, 640), wl['nb'], seed=5, pad_frac=0.02, time_sorted=True)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    c = _c3_grid(dev, seed=13)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    times = torch.cat((torch.tensor([0.41]), torch.linspace(0, 1, wl['nb'] + 1)[:-1] + 0.5 / wl['nb'])).to(dev)
    res = []
    for fused in (True, False):
        cg = c.clone().requires_grad_(True)
        traj = utils.trajectories_from_grid(cg, times, 3, 'polynomial', 4)[0] if fused else _mirror(cg, times, 3, 'polynomial', 4)
        loss, _, _ = L.calc(traj, times, batch)
        loss.backward()
        res.append((loss.item(), cg.grad))
    (lf, gf), (lm, gm) = res
    assert abs(lf - lm) <= 1e-5 * abs(lm)
    assert _rel_l2(gf, gm) <= 1e-4


def test_abi_refuses_bad_arguments_without_launching():
    from motionpriorcmax_amd import ops, _lib as C
    dev = _dev()
    x = torch.zeros(1 << 16, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    L = C.lib()
    with ops.KernelTimer() as kt:
        # k = 17
        assert L.mpc_grid_traj_fwd(vp(x), vp(x), None, C.BASIS_POLY, 0.0, 1, vp(x), None, 1, 1, 17, 8, 8, 4, 2, None) == C.E_UNSUPPORTED
        assert b'basis orders' in L.mpc_last_error_string()
        assert L.mpc_grid_traj_bwd(vp(x), vp(x), None, C.BASIS_DCT, 0.0, None, vp(x), None, None, 1, 1, 17, 8, 8, 4, 2, None) == C.E_UNSUPPORTED
        # a null pointer
        assert L.mpc_grid_traj_fwd(None, vp(x), None, C.BASIS_POLY, 0.0, 1, vp(x), None, 1, 1, 3, 8, 8, 4, 2, None) == C.E_NULL
        assert b'null' in L.mpc_last_error_string()
        assert L.mpc_grid_traj_fwd(vp(x), None, None, C.BASIS_DCT, 0.0, 1, vp(x), None, 1, 1, 3, 8, 8, 4, 2, None) == C.E_NULL
        assert L.mpc_grid_traj_fwd(vp(x), vp(x), None, C.BASIS_MATRIX, 0.0, 1, vp(x), None, 1, 1, 3, 8, 8, 4, 2, None) == C.E_NULL
        assert L.mpc_grid_traj_bwd(vp(x), vp(x), vp(x), C.BASIS_MATRIX, 0.0, None, vp(x), vp(x), vp(x), 1, 1, 3, 8, 8, 4, 2, None) == C.E_NULL
        # a bad tile
        assert L.mpc_grid_traj_fwd(vp(x), vp(x), None, C.BASIS_POLY, 0.0, 1, vp(x), None, 1, 1, 3, 8, 8, 0, 2, None) == C.E_SHAPE
        assert b'tile' in L.mpc_last_error_string()
        assert L.mpc_grid_traj_bwd(vp(x), vp(x), None, C.BASIS_POLY, 0.0, None, vp(x), None, None, 1, 1, 3, 8, 8, -1, 2, None) == C.E_SHAPE
        assert L.mpc_grid_traj_scratch_floats(1, 3, 8, 8, 0, 2) == C.E_SHAPE
        # an unknown basis, and B = 0 (nothing to do)
        assert L.mpc_grid_traj_fwd(vp(x), vp(x), None, 7, 0.0, 1, vp(x), None, 1, 1, 3, 8, 8, 4, 2, None) == C.E_UNSUPPORTED
        assert L.mpc_grid_traj_fwd(vp(x), vp(x), None, C.BASIS_POLY, 0.0, 1, vp(x), None, 0, 1, 3, 8, 8, 4, 2, None) == 0
    assert kt.summary() == {}


def test_flow_from_grid_is_calculate_flow():
    """calculate_flow (trajectory_net.py:121-140) on the device against the oracle's dense flow of the mirror's displacement."""
    from motionpriorcmax_amd import utils
    from oracle import flow_oracle as FO
    g = load_golden('g5a_dct3_l2')
    dev = _dev()
    k, patch, shape = int(g['num_basis']), int(g['patch']), g['cfg']['image_shape']
    cg = torch.from_numpy(g['coeff_grid'])
    got = utils.flow_from_grid(cg.to(dev), k, 'dct', patch, shape)
    disp = _mirror(cg, torch.tensor([1.0]), k, 'dct', patch, add_offsets=False)
    pos = torch.nonzero(utils.get_optical_flow_tile_mask(shape, patch))
    want, _ = FO.dense_flow_from_traj(disp[:, 0], pos, patch, shape)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=2e-5)
