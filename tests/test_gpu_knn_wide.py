"""More than 65535 trajectories per sample (needs an MI355X): the chunked KNN route -- mpc_knn_lut_fwd per contiguous index chunk,
mpc_knn_merge_fwd, mpc_knn_idx_bwd (csrc/knn_wide.hip, ops.knn_wide_fwd) -- through FocusLoss.calc, KnnLutFn and knn_indices.

Inputs are raw point sets (tests/knn_wide_cases.py): image 96 x 128, cells of 4 px (768 queries per bin), a new uniform draw for
every row.  References: brute force by (fp32 distance, index) for the neighbour lists, which must agree EXACTLY; the oracle's
interpolation (focus.py:115-180) in float64 for the LUT -- flows between two independent draws reach 130 px, where one fp32 ulp is
7.6e-6 and the float32 oracle itself is 1.5e-5 to 2.5e-5 off ('iwd'; 7.6e-6 'mean') -- on fixtures whose neighbour sets do not depend
on rounding (tests/test_knn_wide_host.py); the existing 16-bit kernels on a point set both routes serve.
Bounds are the project's: loss rel 1e-5, LUT atol 1e-5, IWE atol 1e-5 x max, gradients by relative L2."""
import pytest
import torch

import knn_wide_cases as KC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cfg(K, nb, T=1, norm='l2', scheme='mean', smooth_type='on_flow_to_tref', smooth_weight=0.003, **kw):
    one = T == 1
    cfg = dict(image_shape=(KC.H, KC.W), num_tref=T, num_bins=nb, num_knn=K, smooth_weight=smooth_weight, lut_superpixel_size=KC.SP,
               focus_loss_norm='l2', dist_norm=norm, scale_iwe_by_dt=one, mask_image_border=True, polarity_aware_batching=one,
               interpolation_scheme=scheme, smooth_type=smooth_type)
    cfg.update(kw)
    return cfg


def _loss(**kw):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', _cfg(**kw))


# ---- 1. the whole loss ---------------------------------------------------------------------------------------------------------
def test_focus_loss_calc_with_65536_trajectories():
    """FocusLoss.calc at n = 65536 (two chunks), 2000 events, 'l2' objective (no sign() ambiguity) against FocusLossOracle: its
    interpolation on brute-force neighbours (knn_wide_cases.oracle_lut in float32: interpolate_flow bit for bit), its event path and
    smoothness term, its autograd.  On the parent commit the library refuses the call."""
    from oracle import focus_oracle as O
    traj, K = KC.fixture('n65536_k4')
    nb = traj.shape[1] - 1
    cfg = _cfg(K, nb)
    ev, num_pos = O.synth_events(1, 2000, (KC.H, KC.W), nb, seed=4, pad_frac=0.02)
    times = torch.cat((torch.tensor([0.41]), O.bin_mid_times(nb)))
    to = traj.clone().requires_grad_(True)
    Lo = O.FocusLossOracle(**cfg)
    lut, _, _ = KC.oracle_lut(to, 1, K, dtype=torch.float32)
    fo, iwo, _ = Lo.event_path(ev, lut, times[:1], num_pos)
    lo = fo + Lo.smooth_loss(lut, None)
    lo.backward()
    lo, fo, iwo = lo.detach(), fo.detach(), iwo.detach()
    tg = traj.to(DEV).requires_grad_(True)
    lg, log, misc = _loss(K=K, nb=nb).calc(tg, times.to(DEV), {'events': ev.to(DEV), 'num_pos_events': num_pos})
    lg.backward()
    iw = misc['iwes'].cpu().reshape(iwo.shape)
    print(f'loss rel {abs(lg.item() - lo.item()) / abs(lo.item()):.2e}  IWE max diff / max {float((iw - iwo).abs().max() / iwo.max()):.2e}  '
          f'gradient rel-L2 {_rel_l2(tg.grad, to.grad):.2e}')
    assert abs(lg.item() - lo.item()) <= 1e-5 * abs(lo.item())
    assert abs(log['focus_loss'].item() - fo.item()) <= 1e-5 * abs(fo.item())
    assert float((iw - iwo).abs().max()) <= 1e-5 * float(iwo.max())
    assert _rel_l2(tg.grad, to.grad) < 1e-4


# ---- 2. neighbour lists ----------------------------------------------------------------------------------------------------------
_BRUTE = {}


def _index_case(n, norm, dup):
    """Two bins of n points (a draw per row) on the device and their ordered 32 nearest by brute force there, computed once; the
    lists of K = 1 and 4 are prefixes."""
    from motionpriorcmax_amd import ops
    key = (n, norm, dup)
    if key not in _BRUTE:
        traj = KC.raw_trajectories(n, 1, 2, seed=100 + n % 89)
        if dup:
            traj = KC.with_duplicates(traj, ops.knn_chunk_starts(n, 32))
        td = traj.to(DEV)
        _BRUTE[key] = (td, torch.stack([KC.brute_knn(td[0, 1 + t], 32, norm)[0] for t in range(2)]))
    return _BRUTE[key]


@pytest.mark.parametrize('K', [1, 4, 32])
@pytest.mark.parametrize('norm', ['l2', 'l1'])
@pytest.mark.parametrize('n,dup', [(65536, False), (65537, False), (70001, False), (131071, False), (131072, False), (131072, True)])
def test_knn_indices_equal_fp32_brute_force(n, dup, norm, K):
    """knn_indices as ordered lists against brute force by (fp32 distance, index): two and three chunks, sizes around the chunk
    limits, and exact duplicates across every chunk boundary (and points 0 and n - 1) that only the index ranks."""
    from motionpriorcmax_amd import ops
    td, want = _index_case(n, norm, dup)
    got = ops.knn_indices(_loss(K=K, nb=2, norm=norm)._cfg, td)
    assert got.shape == (1, 2, 768, K) and got.dtype == torch.int32
    assert torch.equal(got[0].long(), want[:, :, :K])
    if dup and K > 1:
        for qi, a, b in KC.duplicate_pairs(n, ops.knn_chunk_starts(n, 32)):
            assert got[0, :, qi, :2].tolist() == [[a, b], [a, b]]


# ---- 3. the LUT ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,T,scheme,norm,nxt', [('n65536_k4', 1, 'mean', 'l2', True), ('n70001_k32', 1, 'iwd', 'l2', True),
                                                     ('n70001_k32', 3, 'mean', 'l1', False), ('n131072_k32', 3, 'iwd', 'l2', False),
                                                     ('n65536_k4_b2', 1, 'iwd', 'l1', True)])
def test_knn_lut_within_1e5_of_the_oracle(name, T, scheme, norm, nxt):
    """KnnLutFn: LUT and flow_to_next within atol 1e-5 of the oracle's interpolation in float64 -- 'mean' and 'iwd', one and three
    reference times, two and three chunks, B = 2."""
    from motionpriorcmax_amd import ops
    traj, K = KC.fixture(name, T)
    nb = traj.shape[1] - T
    L = _loss(K=K, nb=nb, T=T, norm=norm, scheme=scheme, smooth_type='on_flow_to_next' if nxt else 'on_flow_to_tref')
    lut, fnext = ops.KnnLutFn.apply(traj.to(DEV), L._cfg)
    want, want_next, _ = KC.oracle_lut(traj, T, K, norm, scheme, nxt)
    d = float((lut.cpu().double() - want).abs().max())
    dn = float((fnext.cpu().double() - want_next).abs().max()) if nxt else 0.0
    print(f'{name} T={T} {scheme} {norm}: LUT max diff {d:.2e}, flow_to_next {dn:.2e}')
    assert lut.shape == want.shape and d < 1e-5
    assert (fnext.shape == want_next.shape and dn < 1e-5) if nxt else fnext.numel() == 0


# ---- 4. the backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,T,scheme,nxt', [('n65536_k4', 1, 'mean', False), ('n70001_k32', 1, 'iwd', False), ('n65536_k4', 1, 'mean', True),
                                               ('n65536_k4_b2', 3, 'iwd', False)])
def test_knn_lut_backward_over_the_reported_indices(name, T, scheme, nxt):
    """KnnLutFn backward against float64 autograd through a gather over the neighbour lists the device reports (held to brute force
    above): rel-L2 1e-5; two runs bit for bit; a point in no list gets exactly zero."""
    from motionpriorcmax_amd import ops
    traj, K = KC.fixture(name, T)
    B, nb, n = traj.shape[0], traj.shape[1] - T, traj.shape[2]
    L = _loss(K=K, nb=nb, T=T, scheme=scheme, smooth_type='on_flow_to_next' if nxt else 'on_flow_to_tref')
    g = torch.Generator().manual_seed(7)
    c_lut = torch.randn(B, nb, 24, 32, T, 2, generator=g)
    c_next = torch.randn(B, nb - 1, 24, 32, 1, 2, generator=g) * 3
    grads = []
    for _ in range(2):
        tg = traj.to(DEV).requires_grad_(True)
        lut, fnext = ops.KnnLutFn.apply(tg, L._cfg)
        obj = (lut * c_lut.to(DEV)).sum() + ((fnext * c_next.to(DEV)).sum() if nxt else 0)
        obj.backward()
        grads.append(tg.grad)
    assert torch.equal(grads[0], grads[1])
    idx = ops.knn_indices(L._cfg, traj.to(DEV)).cpu().long()                        # [B, nb, Q, K]
    tc = traj.double().requires_grad_(True)
    q = KC.query_points().double()
    obj = 0
    for b in range(B):
        for t in range(nb):
            i = idx[b, t]
            f = (tc[b, :T].permute(1, 0, 2) - tc[b, T + t][:, None, :])[i]          # [Q, K, T, 2]
            if scheme == 'mean':
                val = f.mean(1)
            else:
                dk = ((q[:, None, :] - tc[b, T + t].detach()[i]) ** 2).sum(-1)
                w = 1 / (dk + 1e-9)
                val = ((w / w.sum(1, keepdim=True))[..., None, None] * f).sum(1)
            obj = obj + (val * c_lut[b, t].reshape(768, T, 2).double()).sum()
            if nxt and t < nb - 1:
                obj = obj + ((tc[b, T + t + 1] - tc[b, T + t])[i].mean(1) * c_next[b, t].reshape(768, 2).double()).sum()
    obj.backward()
    rel = _rel_l2(grads[0], tc.grad)
    print(f'{name} T={T} {scheme} next={nxt}: gradient rel-L2 {rel:.2e}')
    assert rel < 1e-5
    for b in range(B):
        unused = torch.ones(n, dtype=torch.bool)
        unused[idx[b].reshape(-1)] = False
        assert int(unused.sum()) > 1000 and float(grads[0][b][:, unused.to(DEV)].abs().max()) == 0.0


# ---- 5. differential against the 16-bit kernels ----------------------------------------------------------------------------------
@pytest.mark.parametrize('K,scheme', [(4, 'mean'), (4, 'iwd')])
def test_chunked_route_equals_the_native_kernels(monkeypatch, K, scheme):
    """n = 40000 natively and again with KNN_CHUNK lowered to 16384 (three chunks): both routes are exact with one tie rule, so the
    neighbour lists are equal; LUT and flow_to_next within atol 1e-5, the trajectory gradient within rel-L2 1e-5.
    'iwd': the 16-bit kernels sum weights and weighted flows in fp32, which on these 100 px flows (ulp 7.6e-6) leaves THEM 2.3e-5 from
    the float64 oracle (measured; the chunked route: 3.8e-6, half an ulp) -- so there the LUT of each route is held against the
    oracle, the chunked one to the 1e-5 of the issue, and the direct comparison covers neighbour lists, flow_to_next and gradient."""
    from motionpriorcmax_amd import ops
    traj = KC.raw_trajectories(40000, 1, 2, seed=40).to(DEV)
    L = _loss(K=K, nb=2, scheme=scheme, smooth_type='on_flow_to_next')
    g = torch.Generator().manual_seed(8)
    c_lut, c_next = torch.randn(1, 2, 24, 32, 1, 2, generator=g).to(DEV), torch.randn(1, 1, 24, 32, 1, 2, generator=g).to(DEV)
    calls = []
    real_call = ops._call
    monkeypatch.setattr(ops, '_call', lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])

    def run():
        del calls[:]
        tg = traj.clone().requires_grad_(True)
        lut, fnext = ops.KnnLutFn.apply(tg, L._cfg)
        ((lut * c_lut).sum() + (fnext * c_next).sum()).backward()
        return ops.knn_indices(L._cfg, traj), lut.detach(), fnext.detach(), tg.grad, list(calls)
    native = run()
    assert 'mpc_knn_merge_fwd' not in native[4] and 'mpc_knn_lut_bwd' in native[4]
    monkeypatch.setattr(ops, 'KNN_CHUNK', 16384)
    wide = run()
    assert wide[4].count('mpc_knn_merge_fwd') == 2 and wide[4].count('mpc_knn_lut_fwd') == 6 and 'mpc_knn_idx_bwd' in wide[4]
    d, dn, rel = float((wide[1] - native[1]).abs().max()), float((wide[2] - native[2]).abs().max()), _rel_l2(wide[3], native[3])
    print(f'K={K} {scheme}: LUT max diff {d:.2e}, flow_to_next {dn:.2e}, gradient rel-L2 {rel:.2e}')
    assert torch.equal(wide[0], native[0])
    assert dn < 1e-5 and rel < 1e-5
    if scheme == 'mean':
        assert d < 1e-5
    else:
        want, _, _ = KC.oracle_lut(traj.cpu(), 1, K, 'l2', scheme)
        dw, dnat = float((wide[1].cpu().double() - want).abs().max()), float((native[1].cpu().double() - want).abs().max())
        print(f'K={K} {scheme}: from the float64 oracle: chunked {dw:.2e}, native {dnat:.2e}')
        assert dw < 1e-5


def test_chunked_route_reports_the_native_indices_at_k32(monkeypatch):
    """The same differential for the neighbour lists alone at K = 32, 'l1' distance."""
    from motionpriorcmax_amd import ops
    traj = KC.raw_trajectories(40000, 1, 2, seed=41).to(DEV)
    L = _loss(K=32, nb=2, norm='l1')
    native = ops.knn_indices(L._cfg, traj)
    monkeypatch.setattr(ops, 'KNN_CHUNK', 16384)
    assert torch.equal(ops.knn_indices(L._cfg, traj), native)


# ---- 6. routing ------------------------------------------------------------------------------------------------------------------
def test_65535_trajectories_take_the_native_route(monkeypatch):
    """n = 65535: the 16-bit kernels, the fused call, no merge; static_shapes / pyramid_levels with n = 65536 name the limit."""
    from motionpriorcmax_amd import ops
    from oracle import focus_oracle as O
    calls = []
    real_call = ops._call
    monkeypatch.setattr(ops, '_call', lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    traj = KC.raw_trajectories(65536, 1, 2, seed=6).to(DEV)
    ev, num_pos = O.synth_events(1, 500, (KC.H, KC.W), 2, seed=1)
    times = torch.cat((torch.tensor([0.3]), O.bin_mid_times(2))).to(DEV)
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    L = _loss(K=4, nb=2)
    t1 = traj[:, :, :65535].contiguous().requires_grad_(True)
    L.calc(t1, times, batch)[0].backward()
    ops.knn_indices(L._cfg, t1.detach())
    ops.KnnLutFn.apply(t1.detach(), L._cfg)
    assert 'mpc_focus_fwd' in calls and 'mpc_focus_bwd' in calls and 'mpc_knn_lut_fwd' in calls
    assert not [c for c in calls if c in ('mpc_knn_merge_fwd', 'mpc_knn_idx_bwd')]
    del calls[:]
    t2 = traj.clone().requires_grad_(True)
    L.calc(t2, times, batch)[0].backward()
    assert 'mpc_knn_merge_fwd' in calls and 'mpc_knn_idx_bwd' in calls and 'mpc_focus_fwd' not in calls
    for kw in (dict(static_shapes=True), dict(pyramid_levels=2)):
        with pytest.raises(ValueError, match='65535'):
            _loss(K=4, nb=2, **kw).calc(traj, times, batch)


@pytest.mark.parametrize('scheme', ['mean'])
def test_num_tref_2_on_both_settings_of_trefs_as_samples(scheme):
    """num_tref = 2 at n = 65536: the reference times as samples of the num_tref == 1 kernels against the general kernels -- two
    routes into the same chunked search: loss 2e-6, images 1e-5 x max, gradient 1e-4 (the bounds of test_gpu_fullsize.py)."""
    from oracle import focus_oracle as O
    traj, K = KC.fixture('n65536_k4', T=2)
    nb = traj.shape[1] - 2
    ev, _ = O.synth_events(1, 2000, (KC.H, KC.W), nb, seed=5)
    times = torch.cat((torch.tensor([0.0, 1.0]), O.bin_mid_times(nb))).to(DEV)
    outs = []
    for as_samples in (True, False):
        L = _loss(K=K, nb=nb, T=2, scheme=scheme, trefs_as_samples=as_samples)
        t = traj.to(DEV).requires_grad_(True)
        loss, log, misc = L.calc(t, times, {'events': ev.to(DEV)})
        loss.backward()
        outs.append((loss.item(), misc['iwes'], t.grad))
    a, g = outs
    assert a[1].shape == g[1].shape == (1, 2, KC.H, KC.W)
    assert abs(a[0] - g[0]) <= 2e-6 * abs(g[0])
    assert float((a[1] - g[1]).abs().max()) <= 1e-5 * float(g[1].abs().max())
    assert _rel_l2(a[2], g[2]) < 1e-4
