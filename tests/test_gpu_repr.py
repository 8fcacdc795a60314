"""Centred voxel grid (EVIMO2 / MultiFlow network input, csrc/repr.hip): the HIP path against the reference's golden vectors
and the CPU oracle, everything through the C ABI.  Tolerances are the ones tests/test_gpu_voxel.py holds the DSEC builder to
(fp32 tap weights, fixed-point sums against the reference's sequential fp32 put_)."""
import numpy as np
import pytest
import torch

from test_repr_oracle import FULL_INPUTS, REPR_CASES, RESIZE_TO, full_sample, load_repr

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


def _pad(samples, dev, float_xy=False):
    """[(x, y, p, t)] of different lengths (+ empty ones) -> padded [B, N] device tensors in the ABI's dtypes, counts."""
    N = max(int(s[3].numel()) for s in samples)
    B = len(samples)
    x, y, p = (torch.zeros(B, N) for _ in range(3))
    t = torch.zeros(B, N, dtype=torch.int64)
    for b, (xs, ys, ps, ts) in enumerate(samples):
        n = ts.numel()
        x[b, :n], y[b, :n], p[b, :n], t[b, :n] = xs.float(), ys.float(), ps.float(), ts
    if not float_xy:
        x, y = x.int(), y.int()
    counts = torch.tensor([int(s[3].numel()) for s in samples], dtype=torch.int32)
    return x.to(dev), y.to(dev), p.to(dev), t.to(dev), counts.to(dev)


def _close(out, ref, what):
    """The rule of test_voxel_batched_ragged_full_size_vs_oracle: at most 2 entries beyond 5e-6 * max(1, |ref|max)."""
    scale = max(1.0, float(ref.abs().max()))
    diff = (out - ref).abs()
    bad = int((diff > 5e-6 * scale).sum())
    print(f'{what}: max diff {float(diff.max()):.3e}, |ref|max {scale:.2f}, entries beyond the bound {bad}')
    assert bad <= 2, (what, float(diff.max()))


@pytest.mark.parametrize('name', REPR_CASES)
def test_repr_golden(name):
    from motionpriorcmax_amd.utils import representation as P, representation_grids
    g = load_repr(name)
    dev = _dev()
    x, y, p, t = (torch.from_numpy(g[k]).to(dev) for k in ('x', 'y', 'pol', 'time'))
    c = g['centres'] or (None, None)
    vg = P.VoxelGrid(*g['shape'])
    raw = vg.convert(x, y, p, t, *c)
    assert raw.shape == g['raw'].shape
    np.testing.assert_allclose(raw.cpu().numpy(), g['raw'], rtol=0, atol=2e-6 * max(1.0, np.abs(g['raw']).max()))
    if name.startswith('g12_repr_e'):
        assert not raw.cpu().numpy()[g['raw'] == 0].any()                   # exactly zero where the reference is zero
    cnt = torch.tensor([t.numel()], dtype=torch.int32, device=dev)
    if 'normed' in g:
        atol = 2e-6 * max(1.0, np.abs(g['normed']).max())
        normed = P.norm_voxel_grid(raw.clone()).cpu().numpy()
        fused = representation_grids(x[None], y[None], p[None], t[None], cnt, *g['shape'], centres=g['centres'], normalize=True)[0].cpu().numpy()
        for out in (normed, fused):
            np.testing.assert_allclose(out, g['normed'], rtol=0, atol=atol)
            if name.startswith('g12_repr_e'):
                assert not out[g['normed'] == 0].any()                  # exactly zero where the reference is zero
    if 'resized' in g:
        out = representation_grids(x[None], y[None], p[None], t[None], cnt, *g['shape'], centres=g['centres'], normalize=True,
                                   out_size=RESIZE_TO[name])[0].cpu().numpy()
        assert out.shape == g['resized'].shape
        np.testing.assert_allclose(out, g['resized'], rtol=0, atol=2e-6 * max(1.0, np.abs(g['resized']).max()))


def _evimo2_batch(dev):
    shape = FULL_INPUTS['evimo2'][0]
    samples = [full_sample('evimo2', k)[:4] for k in range(2)]
    e = torch.zeros(0, dtype=torch.int32)
    samples.append((e, e, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
    return shape, samples, _pad(samples, dev)


def test_repr_evimo2_full_size_vs_oracle():
    """65 x 480 x 640, ragged batch 1 500 000 / 800 000 / 0 events, default centres: raw, normalised, normalised + resized."""
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape, samples, (x, y, p, t, cnt) = _evimo2_batch(dev)
    raw = representation_grids(x, y, p, t, cnt, *shape).cpu()
    normed = representation_grids(x, y, p, t, cnt, *shape, normalize=True).cpu()
    resized = representation_grids(x, y, p, t, cnt, *shape, normalize=True, out_size=(384, 512)).cpu()
    assert raw.shape == (3, 65, 480, 640) and resized.shape == (3, 65, 384, 512)
    for b in range(2):
        ref = R.voxel_grid(*samples[b], shape)
        _close(raw[b], ref, f'raw[{b}]')
        ref = R.norm_voxel_grid(ref)
        _close(normed[b], ref, f'normalised[{b}]')
        _close(resized[b], R.resize_bilinear(ref, (384, 512)), f'resized[{b}]')
    for out in (raw, normed, resized):
        assert not out[2].any()                                         # the empty sample


def test_repr_multiflow_centres_tensor_vs_oracle():
    """Explicit centres as a [B, 2] device tensor, events of the extended window, 65 x 384 x 512, normalised."""
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape = FULL_INPUTS['multiflow'][0]
    full = [full_sample('multiflow', k) for k in range(2)]
    x, y, p, t, cnt = _pad([f[:4] for f in full], dev)
    centres = torch.tensor([f[4] for f in full], dtype=torch.int64, device=dev)
    out = representation_grids(x, y, p, t, cnt, *shape, centres=centres, normalize=True).cpu()
    for b, f in enumerate(full):
        assert int(f[3][0]) < f[4][0] and int(f[3][-1]) > f[4][1]       # events before the first and after the last centre
        _close(out[b], R.norm_voxel_grid(R.voxel_grid(*f[:4], shape, *f[4])), f'multiflow[{b}]')


def test_repr_float_xy_vs_oracle():
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape = FULL_INPUTS['float_xy'][0]
    x, y, p, t, c = full_sample('float_xy', 0)
    X, Y, P, T, cnt = _pad([(x, y, p, t)], dev, float_xy=True)
    ref = R.voxel_grid(x, y, p, t, shape, *c)
    _close(representation_grids(X, Y, P, T, cnt, *shape, centres=c).cpu()[0], ref, 'float raw')
    ref = R.norm_voxel_grid(ref)
    _close(representation_grids(X, Y, P, T, cnt, *shape, centres=c, normalize=True).cpu()[0], ref, 'float normalised')
    _close(representation_grids(X, Y, P, T, cnt, *shape, centres=c, normalize=True, out_size=(96, 128)).cpu()[0],
           R.resize_bilinear(ref, (96, 128)), 'float resized')


@pytest.mark.parametrize('out_size', [(360, 480), (400, 498), (600, 800)])
def test_repr_resize_strips_share_rows(out_size):
    """Resize factors at which neighbouring strips of output rows interpolate from common input rows (480 -> 384 with 12-row
    strips happens to cut at whole input rows): one shared row when shrinking, up to two when growing; a width that is not a
    multiple of 4 takes the 4-byte store path.  Sample 1 of the guarded EVIMO2 inputs."""
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape = FULL_INPUTS['evimo2'][0]
    sample = full_sample('evimo2', 1)[:4]
    x, y, p, t, cnt = _pad([sample], dev)
    ref = R.norm_voxel_grid(R.voxel_grid(*sample, shape))
    out = representation_grids(x, y, p, t, cnt, *shape, normalize=True, out_size=out_size).cpu()[0]
    _close(out, R.resize_bilinear(ref, out_size), f'resized to {out_size}')


@pytest.mark.parametrize('out_size', [(97, 131), (150, 200)])
def test_repr_float_xy_resize_strips_share_rows(out_size):
    """The eight-tap path with rows y0, y0 + 1 on both sides of a strip boundary and in shared rows."""
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape = FULL_INPUTS['float_xy'][0]
    x, y, p, t, c = full_sample('float_xy', 0)
    X, Y, P, T, cnt = _pad([(x, y, p, t)], dev, float_xy=True)
    ref = R.norm_voxel_grid(R.voxel_grid(x, y, p, t, shape, *c))
    out = representation_grids(X, Y, P, T, cnt, *shape, centres=c, normalize=True, out_size=out_size).cpu()[0]
    _close(out, R.resize_bilinear(ref, out_size), f'float resized to {out_size}')


def test_repr_bucket_overflow():
    """All events in two rows and two time slices: the per-bucket capacity overflows into the spill list."""
    from motionpriorcmax_amd.utils import representation_grids
    from oracle import repr_oracle as R
    dev = _dev()
    shape = (65, 480, 640)
    n = 200000
    x, y, p, t = R.synth_int_events(n, shape, 0, 1000000, 50)
    y = (100 + (y % 2)).int()
    t = torch.sort(500000 + t // 200).values                           # 5 000 us of a 1 000 000 us window: under one channel step
    c = (0, 1000000)
    ref = R.voxel_grid(x, y, p, t, shape, *c)
    assert int((ref != 0).any(-1).any(-1).sum()) == 2 and int((ref != 0).any(0).any(-1).sum()) == 2
    X, Y, P, T, cnt = _pad([(x, y, p, t)], dev)
    out = representation_grids(X, Y, P, T, cnt, *shape, centres=c).cpu()[0]
    np.testing.assert_allclose(out.numpy(), ref.numpy(), atol=1e-4)
    out = representation_grids(X, Y, P, T, cnt, *shape, centres=c, out_size=(384, 512)).cpu()[0]
    np.testing.assert_allclose(out.numpy(), R.resize_bilinear(ref, (384, 512)).numpy(), atol=1e-4)


def test_repr_reproducible_and_batch_independent():
    from motionpriorcmax_amd.utils import representation_grids
    dev = _dev()
    shape, samples, (x, y, p, t, cnt) = _evimo2_batch(dev)
    kw = dict(normalize=True, out_size=(384, 512))
    a = representation_grids(x, y, p, t, cnt, *shape, **kw)
    b = representation_grids(x, y, p, t, cnt, *shape, **kw)
    assert torch.equal(a, b)
    n1 = int(cnt[1])
    alone = representation_grids(x[1:2, :n1].contiguous(), y[1:2, :n1].contiguous(), p[1:2, :n1].contiguous(), t[1:2, :n1].contiguous(),
                                 cnt[1:2], *shape, **kw)
    assert torch.equal(alone[0], a[1])


def _small_batch(dev, seed):
    from oracle import repr_oracle as R
    shape = (9, 60, 80)
    samples = [R.synth_int_events(n, shape, 1000, 900000, seed + i) for i, n in enumerate((30000, 12000))]
    return shape, _pad(samples, dev)


def test_repr_no_host_sync_and_graph_capture():
    from motionpriorcmax_amd.utils import representation_grids
    dev = _dev()
    shape, (x, y, p, t, cnt) = _small_batch(dev, 20)
    centres = torch.tensor([[1000, 900000], [5000, 800000]], dtype=torch.int64, device=dev)
    kw = dict(normalize=True, out_size=(48, 64))
    representation_grids(x, y, p, t, cnt, *shape, centres=centres, **kw)           # one-time set-up outside the checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        representation_grids(x, y, p, t, cnt, *shape, centres=centres, **kw)
        representation_grids(x, y, p, t, cnt, *shape, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    # capture, then replay twice with refilled inputs
    _, fresh = _small_batch(dev, 30)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up outside the capture
        representation_grids(x, y, p, t, cnt, *shape, centres=centres, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = representation_grids(x, y, p, t, cnt, *shape, centres=centres, **kw)
    for inputs in ((x.clone(), y.clone(), p.clone(), t.clone(), cnt.clone()), fresh):
        eager = representation_grids(*inputs, *shape, centres=centres, **kw)
        for dst, src in zip((x, y, p, t, cnt), inputs):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        assert out.abs().sum() > 0


def test_repr_int_xy_switch_for_fp32_coordinates():
    """fp32 coordinates that hold integers (the ABI's dtype, no conversion pass) with int_xy=True: the two-tap path, bit for bit."""
    from motionpriorcmax_amd.utils import representation_grids
    dev = _dev()
    shape, (x, y, p, t, cnt) = _small_batch(dev, 60)
    kw = dict(normalize=True, out_size=(48, 64))
    ref = representation_grids(x, y, p, t, cnt, *shape, **kw)
    assert torch.equal(representation_grids(x.float(), y.float(), p, t, cnt, *shape, int_xy=True, **kw), ref)
    eight = representation_grids(x.float(), y.float(), p, t, cnt, *shape, **kw)          # eight taps, six of weight 0: the same grid
    assert float((eight - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


def test_repr_norm_all_entries_equal():
    """Non-zero entries that are all equal but not a power of two (0.3: sums and squares round): the reference's std is 0 and it
    only subtracts the mean; a variance from rounded sums must not turn that into a division by a tiny number."""
    from motionpriorcmax_amd.utils import representation as P, representation_grids
    dev = _dev()
    g = torch.zeros(5, 12, 16, device=dev)
    g[1, 2:9, 3:11] = 0.3
    ref = g.cpu().clone()
    nz = ref != 0
    ref[nz] = ref[nz] - ref[nz].double().mean().float()               # std == 0: the subtract-only branch (representation.py:16-17)
    out = P.norm_voxel_grid(g.clone()).cpu()
    assert float((out - ref).abs().max()) <= 2e-6 and not out[~nz].any()
    # the statistics taken from the strips decide the same way as the plain kernels: 40 events of polarity 1 at one
    # timestamp, 0.7 into channel 1 and 0.3 (rounded) into channel 2 of 40 pixels
    i = torch.arange(40, device=dev)
    x, y = (i % 16).int()[None], (i // 16 + 2).int()[None]
    p = torch.ones(1, 40, dtype=torch.int64, device=dev)
    t = torch.full((1, 40), 2300, dtype=torch.int64, device=dev)
    cnt = torch.tensor([40], dtype=torch.int32, device=dev)
    raw = representation_grids(x, y, p, t, cnt, 5, 12, 16, centres=(1000, 5000))
    fused = representation_grids(x, y, p, t, cnt, 5, 12, 16, centres=(1000, 5000), normalize=True)
    assert float((fused[0] - P.norm_voxel_grid(raw[0].clone())).abs().max()) <= 2e-6       # (squares: fp32 per thread there, fp64 here)
    # all votes in the last channel only (t_norm = C - 1 + 0.7: weight 0.3 rounded, 40 equal entries): std == 0 through the strips
    t = torch.full((1, 40), 5700, dtype=torch.int64, device=dev)
    raw = representation_grids(x, y, p, t, cnt, 5, 12, 16, centres=(1000, 5000))[0].cpu()
    fused = representation_grids(x, y, p, t, cnt, 5, 12, 16, centres=(1000, 5000), normalize=True)[0].cpu()
    nz = raw != 0
    assert int(nz.sum()) == 40 and float(raw[nz].max()) == float(raw[nz].min())
    assert float(fused.abs().max()) <= 2e-6


def test_repr_error_paths():
    from motionpriorcmax_amd.utils import representation as P, representation_grids
    dev = _dev()
    shape, (x, y, p, t, cnt) = _small_batch(dev, 40)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        representation_grids(x.cpu(), y, p, t, cnt, *shape)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        P.VoxelGrid(*shape).convert(x[0].cpu(), y[0].cpu(), p[0].cpu(), t[0].cpu())
    with pytest.raises(TypeError, match='integer'):
        representation_grids(x, y, p, t.float(), cnt, *shape)
    with pytest.raises(ValueError):
        representation_grids(x, y, p, t, cnt, 1, shape[1], shape[2])
    with pytest.raises(AssertionError):
        P.VoxelGrid(1, 60, 80)
    with pytest.raises(ValueError, match='shape'):
        representation_grids(x, y[:, :-1], p, t, cnt, *shape)
    with pytest.raises(NotImplementedError, match='downsample'):
        representation_grids(x, y, p, t, cnt, *shape, downsample=True)
    out = representation_grids(x, y, p, t, cnt, *shape, normalize=False, out_size=(30, 40))          # a resize without the normalisation is allowed
    assert out.shape == (2, 9, 30, 40) and bool(torch.isfinite(out).all()) and float(out.abs().sum()) > 0
    # the C ABI refuses what the reference asserts, with a message
    import ctypes
    from motionpriorcmax_amd import _lib as C
    bad = C.ReprShape(B=1, N=10, C=1, H=60, W=80, int_xy=1, norm=0, Ho=0, Wo=0)
    assert C.lib().mpc_repr_workspace_bytes(ctypes.byref(bad)) == C.E_UNSUPPORTED
    assert b'exceed 1' in C.lib().mpc_last_error_string()
