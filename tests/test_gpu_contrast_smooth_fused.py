"""The LUT smoothness pass inside the contrast launch (k_contrast_smooth_march, mpc_focus_fwd) against the stage-by-stage path,
which launches k_lut_smooth_march and k_contrast_march separately.  The fused kernel runs the two bodies unchanged and writes the
partial sums into the slots the separate launches write, so everything below is compared bit for bit: the three loss scalars,
the blurred images, the adjoint image and the smoothness gradient.

Band heights (contrast.hip): the contrast kernel takes bands of 16 rows instead of 32 below 1536 workgroups
(ceil(W / 56) * ceil(H / 32) * images), the smoothness kernel bands of 8 rows instead of 16 below 1536 workgroups
(ceil(wq / 60) * ceil(hq / 16) * fields).  At 480 x 640 with 4-pixel cells that is 360 contrast workgroups per sample (two
polarity images) and 24 smoothness workgroups per (sample, bin)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FUSED_KERNEL, SMOOTH_KERNEL, CONTRAST_KERNEL = 'k_contrast_smooth_march', 'k_lut_smooth_march', 'k_contrast_march'


def _cfg(shape, nb, **over):
    c = dict(image_shape=shape, num_tref=1, num_bins=nb, num_knn=4, smooth_weight=0.003, lut_superpixel_size=4,
             focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True,
             polarity_aware_batching=True, interpolation_scheme='mean', smooth_type='on_flow_to_tref',
             auto_static_shapes=False)
    c.update(over)
    return c


def _case(shape, B, M, nb, seed, mag=3.0):
    from oracle import focus_oracle as O
    ev, num_pos = O.synth_events(B, M, shape, nb, seed=seed, pad_frac=0.03)
    g = torch.Generator().manual_seed(seed)
    coeff = torch.randn(B, 1, 2, *shape, generator=g) * mag
    times = torch.cat((torch.tensor([0.3]), O.bin_mid_times(nb)))
    traj = O.trajectories_at(coeff, times, O.tile_mask(shape, 4), 1, 'polynomial')
    return ev, num_pos, traj, times


def _forward(L, traj, times, batch, fused, monkeypatch):
    """One forward (+ backward) of L.calc; returns the scalars, the blurred images, the adjoint image, the smoothness gradient
    (None where the step has none), the trajectory gradient and the launches a second, timed forward made."""
    from motionpriorcmax_amd import ops
    monkeypatch.setattr(ops, 'FUSED_CALLS', fused)
    t = traj.clone().requires_grad_(True)
    loss, log, misc = L.calc(t, times, batch)
    fn = loss.grad_fn
    if fused:
        assert fn.plan is not None
        buf = fn.saved_tensors[3]
        gimg, gf = fn.plan.view(buf, 'gimg'), fn.plan.view(buf, 'gf')
    else:
        assert fn.plan is None
        gimg, gf = fn.saved_tensors[5], fn.saved_tensors[7]
    out = dict(loss=loss.detach().clone(), focus=log['focus_loss'].clone(), smooth=log['smoothness_loss'].clone(),
               iwes=misc['iwes'].clone(), gimg=gimg.detach().clone().reshape(-1),
               gf=None if gf is None else gf.detach().clone().reshape(-1))
    loss.backward()
    out['grad'] = t.grad.clone()
    with ops.KernelTimer() as kt:
        L.calc(traj.clone().requires_grad_(True), times, batch)
    out['launches'] = {k: v['launches'] for k, v in kt.summary().items()}
    return out


def _same(a, b):
    for k in ('loss', 'focus', 'smooth', 'iwes', 'gimg', 'gf'):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
    assert torch.isfinite(a['loss']) and a['gimg'].abs().max() > 0


def _both(shape, B, M, nb, seed, monkeypatch, **over):
    from motionpriorcmax_amd import LossFactory
    dev = torch.device('cuda:0')
    ev, num_pos, traj, times = _case(shape, B, M, nb, seed)
    L = LossFactory.get_loss_calculator('FOCUS', _cfg(shape, nb, **over))
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    traj, times = traj.to(dev), times.to(dev)
    one = _forward(L, traj, times, batch, True, monkeypatch)
    two = _forward(L, traj, times, batch, False, monkeypatch)
    _same(one, two)
    # the stage-by-stage path always launches the two kernels separately
    assert two['launches'].get(SMOOTH_KERNEL, 0) == (1 if over.get('smooth_weight', 1) > 0 else 0)
    assert FUSED_KERNEL not in two['launches']
    return one, two


def _assert_fused(one):
    assert one['launches'].get(FUSED_KERNEL) == 1, one['launches']
    assert SMOOTH_KERNEL not in one['launches'] and CONTRAST_KERNEL not in one['launches'], one['launches']


# (B, nb): 360 B contrast workgroups, 24 B nb (on_flow_to_next: 24 B (nb - 1)) smoothness workgroups at 480 x 640
BANDS = {
    'both_below': (1, 15),           # 360, 360 (336)
    'both_above': (5, 15),           # 1800, 1800 (1680)
    'contrast_above': (5, 5),        # 1800, 600 (480)
    'smooth_above': (2, 40),         # 720, 1920 (1872)
}


@pytest.mark.parametrize('norm', ['l1', 'l2'])
@pytest.mark.parametrize('smooth_type', ['on_flow_to_tref', 'on_flow_to_next'])
@pytest.mark.parametrize('bands', sorted(BANDS))
def test_fused_equals_separate_launches(bands, smooth_type, norm, monkeypatch):
    """640 is not a multiple of 56 and wq = 160 not a multiple of 60; every combination of the two band heights."""
    B, nb = BANDS[bands]
    one, _ = _both((480, 640), B, 30000, nb, 11, monkeypatch, focus_loss_norm=norm, smooth_type=smooth_type)
    _assert_fused(one)
    assert one['gf'] is not None and one['gf'].abs().max() > 0


@pytest.mark.parametrize('shape', [(100, 172), (48, 60), (132, 484), (33, 57), (17, 113)])
@pytest.mark.parametrize('smooth_type', ['on_flow_to_tref', 'on_flow_to_next'])
def test_odd_sizes(shape, smooth_type, monkeypatch):
    """Partial tiles in both directions of both grids; one tile column (wq = 15), several (wq = 121 = 2 * 60 + 1); and two
    shapes that tests/test_gpu_contrast_cases.py holds element by element against float64: 33 x 57 (one row and one column past a
    band and a 56-column group) and 17 x 113 (three column groups)."""
    one, _ = _both(shape, 3, 6000, 5, 5, monkeypatch, smooth_type=smooth_type)
    _assert_fused(one)


@pytest.mark.parametrize('smooth_type', ['on_flow_to_tref', 'on_flow_to_next'])
def test_single_lut_column(smooth_type, monkeypatch):
    """32-pixel cells on a 40 x 32 image: hq = 2, wq = 1 -- a smoothness workgroup with one cell column, both neighbours the
    zero padding."""
    one, _ = _both((40, 32), 3, 6000, 5, 5, monkeypatch, smooth_type=smooth_type, lut_superpixel_size=32)
    _assert_fused(one)
    assert one['gf'] is not None and one['gf'].abs().max() > 0


def test_fused_step_launches_neither_separate_kernel(monkeypatch):
    one, two = _both((96, 128), 2, 8000, 5, 3, monkeypatch)
    _assert_fused(one)
    assert two['launches'].get(SMOOTH_KERNEL) == 1 and two['launches'].get(CONTRAST_KERNEL) == 1, two['launches']


def test_fallback_without_smoothness(monkeypatch):
    one, _ = _both((96, 128), 2, 8000, 5, 3, monkeypatch, smooth_weight=0.0)
    assert one['launches'].get(CONTRAST_KERNEL) == 1 and FUSED_KERNEL not in one['launches'] and SMOOTH_KERNEL not in one['launches'], one['launches']
    assert one['gf'] is None and float(one['smooth']) == 0.0


def test_fallback_variance_objective(monkeypatch):
    """The variance objective has no marching kernel: the smoothness launch stays in front of the event forward."""
    one, _ = _both((96, 128), 2, 8000, 5, 3, monkeypatch, loss_type='variance')
    assert one['launches'].get(SMOOTH_KERNEL) == 1 and one['launches'].get('k_contrast_fwd') == 1, one['launches']
    assert FUSED_KERNEL not in one['launches'] and CONTRAST_KERNEL not in one['launches'], one['launches']


def test_fallback_forward_only(monkeypatch):
    """No gradient asked: no adjoint image, the two stage kernels (k_contrast_fwd, k_lut_smooth_march) as before."""
    from motionpriorcmax_amd import LossFactory, ops
    dev = torch.device('cuda:0')
    shape, B, M, nb = (96, 128), 2, 8000, 5
    ev, num_pos, traj, times = _case(shape, B, M, nb, 3)
    L = LossFactory.get_loss_calculator('FOCUS', _cfg(shape, nb))
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    traj, times = traj.to(dev), times.to(dev)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, 'FUSED_CALLS', fused)
        with ops.KernelTimer() as kt:
            loss, log, misc = L.calc(traj, times, batch)
        res[fused] = (loss.clone(), log['focus_loss'].clone(), log['smoothness_loss'].clone(), misc['iwes'].clone())
        names = kt.summary()
        assert FUSED_KERNEL not in names and names[SMOOTH_KERNEL]['launches'] == 1 and names['k_contrast_fwd']['launches'] == 1, names
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('smooth_type', ['on_flow_to_tref', 'on_flow_to_next'])
def test_static_shapes(smooth_type, monkeypatch):
    """The captured plan replays mpc_focus_fwd: same scalars, images and trajectory gradient as the eager fused step, and the
    scalars and images of the stage-by-stage path."""
    from motionpriorcmax_amd import LossFactory, ops
    dev = torch.device('cuda:0')
    shape, B, M, nb = (100, 172), 2, 8000, 5
    ev, num_pos, traj, times = _case(shape, B, M, nb, 9)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    traj, times = traj.to(dev), times.to(dev)
    Ls = LossFactory.get_loss_calculator('FOCUS', _cfg(shape, nb, smooth_type=smooth_type, static_shapes=True))
    Le = LossFactory.get_loss_calculator('FOCUS', _cfg(shape, nb, smooth_type=smooth_type))

    def step(L):
        t = traj.clone().requires_grad_(True)
        loss, log, misc = L.calc(t, times, batch)
        loss.backward()
        return loss.detach().clone(), log['focus_loss'].clone(), log['smoothness_loss'].clone(), misc['iwes'].clone(), t.grad.clone()

    monkeypatch.setattr(ops, 'FUSED_CALLS', True)
    step(Ls)                                    # (captures)
    stat = step(Ls)                             # (replays)
    eager = step(Le)
    monkeypatch.setattr(ops, 'FUSED_CALLS', False)
    stage = step(Le)
    for a, b in zip(stat, eager):
        assert torch.equal(a, b)
    for a, b in zip(stat[:4], stage[:4]):
        assert torch.equal(a, b)
    assert stat[4].abs().max() > 0
