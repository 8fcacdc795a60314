"""The IWE pyramid served on every loss route by one fused pass (csrc/iwe_pyramid.hip, ops.iwe_pyramid_pass): the pass alone per
element against its float64 definition and against the stage calls it replaces, the per-event routes (which ignored
`pyramid_levels` before the pass existed) against the definition, `calc` across event layouts, the captured plan and the
stage-call route, launch counts, no host synchronisation, and the refusals.  Cases and definition: tests/iwe_pyramid_cases.py."""
import ctypes

import pytest
import torch

import iwe_pyramid_cases as PY

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _loss(cfg):
    from motionpriorcmax_amd import LossFactory
    return LossFactory.get_loss_calculator('FOCUS', cfg)


# ---- 1. the pass alone -----------------------------------------------------------------------------------------------------------
def _level_shape(nimg, H, W, norm):
    from motionpriorcmax_amd import ops
    cfg = ops.PathConfig(image_shape=(H, W), num_tref=1, num_bins=1, num_knn=0, smooth_weight=0.0, sp=4, norm_l2=(norm == 'l2'), dist_l1=False,
                         scale_by_dt=False, mask_border=False, polarity_split=False, scheme_iwd=False, smooth_on_next=False)
    return ops.make_shape(cfg, nimg, 0, 0, 0, K=0)


def _stage_level(raw, norm):
    """mpc_contrast_fwd -> mpc_finalize on raw [nimg, 1, H, W]: (unscaled adjoint image, scalars)."""
    from motionpriorcmax_amd import ops
    sh = _level_shape(raw.shape[0], raw.shape[2], raw.shape[3], norm)
    ws = ops.alloc_workspace(sh, raw.device)
    _, g = ops.contrast_fwd(sh, raw, ws, True)
    return sh, g, ops.finalize(sh, 0, 0, 0.0, ws, raw.device)


def _stage_pyramid(raw, levels, norm):
    """The stage calls of ops.PyramidFocusFn: mpc_pool2_fwd -> mpc_contrast_fwd -> mpc_finalize per level, then the
    mpc_pool2_bwd_add chain on copies -> (per-level scalars, per-level adjoint images, the chained level-0 adjoint image)."""
    from motionpriorcmax_amd import ops, _lib as C
    nimg = raw.shape[0]
    cur, gs, scals = raw, [], []
    for lv in range(levels):
        if lv:
            nxt = torch.empty((nimg, 1, cur.shape[2] // 2, cur.shape[3] // 2), dtype=torch.float32, device=raw.device)
            ops._call('mpc_pool2_fwd', raw.device, ops._ptr(cur), ops._ptr(nxt), nimg, cur.shape[2], cur.shape[3])
            cur = nxt
        _, g, sc = _stage_level(cur, norm)
        gs.append(g); scals.append(sc)
    chain = [g.clone() for g in gs]
    for lv in range(levels - 1, 0, -1):
        h, w = chain[lv - 1].shape[2:]
        ops._call('mpc_pool2_bwd_add', raw.device, ops._ptr(chain[lv]), ctypes.c_void_p(scals[lv].data_ptr() + 4 * C.SCAL_GCOEF), ops._ptr(chain[lv - 1]),
                  ctypes.c_void_p(scals[lv - 1].data_ptr() + 4 * C.SCAL_GCOEF), nimg, h, w)
    return scals, gs, chain[0]


def _run_pass(raw, levels, norm, want_grad=True):
    """Level 0 by the stage calls, then the pass -> (level table, adjoint images [level 0 before the pass, the pass's own coarse
    ones], the folded level-0 image, scal after the pass, scal before)."""
    from motionpriorcmax_amd import ops
    sh, g0, scal = _stage_level(raw, norm)
    before, g0_before = scal.clone(), g0.clone()
    lscal, pws = ops.iwe_pyramid_pass(sh, levels, raw, g0 if want_grad else None, scal)
    gl = [g0_before]
    if want_grad:
        fl = pws.view(torch.float32)
        for off, shp in ops.iwe_pyramid_level_offsets(sh, levels):
            n = shp[0] * shp[1] * shp[2]
            gl.append(fl[off:off + n].view(shp[0], 1, shp[1], shp[2]).clone())
    return lscal, gl, g0, scal, before


@pytest.mark.parametrize('norm', ['l2', 'l1'])
@pytest.mark.parametrize('name', list(PY.CASES))
def test_the_pass_alone_per_element(name, norm):
    from motionpriorcmax_amd import _lib as C
    c = PY.CASES[name]
    L = c['levels']
    raw_cpu = PY.raw_images(name)
    raw = raw_cpu[:, None].contiguous().to(DEV)
    lscal, gl, folded, scal, before = _run_pass(raw, L, norm)
    d = PY.definition64(raw_cpu, L, norm)
    st_scal, st_g, st_chain = _stage_pyramid(raw, L, norm)
    ls = lscal.cpu().double()
    # per-level val_l and 1 / val_l: against the float64 definition and against the stage calls, rel 1e-6
    for l in range(L):
        want = float(d['vals'][l])
        st = st_scal[l].cpu().double()
        print(f'case {name} {norm} level {l}: val {float(ls[l, C.SCAL_VAL]):.9g} definition {want:.9g} stage {float(st[C.SCAL_VAL]):.9g}')
        assert abs(float(ls[l, C.SCAL_VAL]) - want) <= 1e-6 * want
        assert abs(float(ls[l, C.SCAL_FOCUS]) - 1 / want) <= 1e-6 / want
        assert abs(float(ls[l, C.SCAL_VAL]) - float(st[C.SCAL_VAL])) <= 1e-6 * want
        assert abs(float(ls[l, C.SCAL_FOCUS]) - float(st[C.SCAL_FOCUS])) <= 1e-6 / want
        assert abs(float(ls[l, C.SCAL_GCOEF]) - float(st[C.SCAL_GCOEF])) <= 2e-6 * abs(float(st[C.SCAL_GCOEF]))
    # scal: focus and loss gained the coarse levels, level 0's VAL and GCOEF stayed
    focus = float(d['focus'])
    assert abs(float(scal[C.SCAL_FOCUS]) - focus) <= 1e-6 * focus and abs(float(scal[C.SCAL_LOSS]) - focus) <= 1e-6 * focus
    assert torch.equal(scal[C.SCAL_VAL:C.SCAL_GCOEF + 1], before[C.SCAL_VAL:C.SCAL_GCOEF + 1]) and torch.equal(lscal[0, :5], before[:5])
    # the pass's coarse adjoint images are the stage calls' (the same marching body on the same bits)
    for l in range(1, L):
        assert torch.equal(gl[l], st_g[l]), l
    # the folded adjoint image per element: against the float64 fold of the kernel's OWN fp32 g_l and level scalars, and against
    # the mpc_pool2_bwd_add chain, both within (2 L + 2) 2^-24 sum_l |r_l g_l|
    want, mag = PY.fold64([g[:, 0] for g in gl], lscal.cpu())
    bound = PY.fold_bound(mag, L)
    keep = torch.ones(want.shape, dtype=torch.bool)
    if norm == 'l1':
        from grad_accounting import pyramid_near_zero_pixels
        keep = ~pyramid_near_zero_pixels(raw_cpu[:, None], L)[:, 0]
        if 'seed' in c:
            assert float((~keep).float().mean()) < PY.MASKED_SHARE_MAX
    got = folded[:, 0].cpu().double()
    chain = st_chain[:, 0].cpu().double()
    e1, e2 = (got - want).abs(), (got - chain).abs()
    print(f'case {name} {norm}: fold against float64 max {float((e1 / bound.clamp_min(1e-300))[keep].max()):.3f} of the bound, against the chain '
          f'{float((e2 / bound.clamp_min(1e-300))[keep].max()):.3f}')
    assert bool((e1 <= bound)[keep].all()) and bool((e2 <= bound)[keep].all())
    assert float(mag.max()) > 0 and float((want - gl[0][:, 0].cpu().double()).abs().max()) > 0          # (the fold added something)
    # the folded image, scaled, is the definition's gradient (sanity of the whole: a relative L2 figure, 'l2' only)
    if norm == 'l2':
        full = float(before[C.SCAL_GCOEF]) * got
        rel = float((full - d['grad']).norm() / d['grad'].norm())
        print(f'case {name}: GCOEF_0 * folded image against the autograd gradient of the definition: rel L2 {rel:.3e}')
        assert rel < 1e-5


@pytest.mark.parametrize('norm', ['l2', 'l1'])
def test_an_all_zero_image_folds_to_zeros(norm):
    from motionpriorcmax_amd import _lib as C
    raw = torch.zeros(2, 1, 16, 24, device=DEV)
    lscal, gl, folded, scal, _ = _run_pass(raw, 3, norm)
    assert not torch.isnan(folded).any() and float(folded.abs().max()) == 0.0
    assert float(lscal[1:, C.SCAL_PYR_RATIO].abs().max()) == 0.0
    # forward only: two launches, the same scalars
    raw2 = PY.raw_images('a')[:, None].contiguous().to(DEV)
    a = _run_pass(raw2, 3, norm, want_grad=True)
    b = _run_pass(raw2, 3, norm, want_grad=False)
    assert torch.equal(a[3], b[3]) and torch.equal(a[0], b[0])


# ---- 2. the per-event routes -----------------------------------------------------------------------------------------------------
PE_SHAPE, PE_B, PE_M, PE_NB = (32, 40), 2, 3000, 5


def _pe_cfg(**over):
    cfg = dict(image_shape=PE_SHAPE, num_tref=1, num_bins=PE_NB, num_knn=8, smooth_weight=0.003, lut_superpixel_size=4, focus_loss_norm='l2',
               dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True, interpolation_scheme='mean',
               smooth_type='on_flow_to_tref')
    cfg.update(over)
    return cfg


def _pe_events():
    from oracle import focus_oracle as O
    return O.synth_events(PE_B, PE_M, PE_SHAPE, PE_NB, seed=11, pad_frac=0.1)


def _check(label, loss, focus, grad, want_loss, want_focus, want_grad):
    rel = float((grad.double().cpu() - want_grad).norm() / want_grad.norm())
    print(f'{label}: loss {float(loss):.8g} / {want_loss:.8g}, focus {float(focus):.8g} / {want_focus:.8g}, gradient rel L2 {rel:.3e}')
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
    assert abs(float(focus) - want_focus) <= 1e-5 * abs(want_focus)
    assert rel < 1e-4


@pytest.mark.parametrize('levels', [2, 3])
@pytest.mark.parametrize('route', ['fused', 'unfused'])
@pytest.mark.parametrize('ordered', [False, True])
def test_per_event_basis_serves_the_pyramid(levels, route, ordered):
    from oracle import focus_oracle as O
    k = 2
    cfg = _pe_cfg()
    ev, num_pos = _pe_events()
    g = torch.Generator().manual_seed(3)
    coeff = torch.randn(PE_B, 1, 2 * k, *PE_SHAPE, generator=g) * 2.0
    co = coeff.double().requires_grad_(True)
    with PY.pyramid_objective(levels):
        lo, logo, _ = O.FocusLossOracle(**cfg).calc_per_event_basis(co, 0.41, {'events': ev.double(), 'num_pos_events': num_pos}, k, 'polynomial')
    lo.backward()
    L = _loss(dict(cfg, pyramid_levels=levels))
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    if ordered:
        batch = L.order_events(batch)
    cg = coeff.to(DEV).requires_grad_(True)
    loss, log, misc = L.calc_per_event_basis(cg, 0.41, batch, k, 'polynomial', fused=(route == 'fused'))
    loss.backward()
    _check(f'per-event basis levels={levels} {route} ordered={ordered}', loss, log['focus_loss'], cg.grad, float(lo), float(logo['focus_loss']), co.grad)
    assert misc['iwes'].shape == (PE_B, 1, 2, *PE_SHAPE)


@pytest.mark.parametrize('levels', [2, 3])
@pytest.mark.parametrize('ordered', [False, True])
def test_per_event_curves_serve_the_pyramid(levels, ordered):
    import pe_curves_cases as PC
    d = 3
    cfg = _pe_cfg()
    ev, num_pos = _pe_events()
    g = torch.Generator().manual_seed(5)
    h, w = PE_SHAPE[0] // 8, PE_SHAPE[1] // 8
    params = torch.randn(PE_B, 2 * d, h, w, generator=g) * 0.3
    mask = torch.randn(PE_B, 576, h, w, generator=g)
    with PY.pyramid_objective(levels):
        r = PC.definition(cfg, ev, num_pos, params, mask, 0.41, 'BEZIER')
    r['loss'].backward()
    L = _loss(dict(cfg, pyramid_levels=levels))
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    if ordered:
        batch = L.order_events(batch)
    pg, mg = params.to(DEV).requires_grad_(True), mask.to(DEV).requires_grad_(True)
    loss, log, _ = L.calc_per_event_curves(pg, 0.41, batch, up_mask=mg, curve_type='BEZIER')
    loss.backward()
    _check(f'per-event curves levels={levels} ordered={ordered} (params)', loss, log['focus_loss'], pg.grad, float(r['loss']), float(r['focus']), r['params'].grad)
    rel = float((mg.grad.double().cpu() - r['mask'].grad).norm() / r['mask'].grad.norm())
    print(f'per-event curves levels={levels}: up_mask gradient rel L2 {rel:.3e}')
    assert rel < 1e-4


def test_one_level_on_the_per_event_routes_is_the_plain_loss_bit_for_bit():
    cfg = _pe_cfg()
    ev, num_pos = _pe_events()
    g = torch.Generator().manual_seed(3)
    coeff = (torch.randn(PE_B, 1, 4, *PE_SHAPE, generator=g) * 2.0).to(DEV)
    params = (torch.randn(PE_B, 6, PE_SHAPE[0] // 8, PE_SHAPE[1] // 8, generator=g) * 0.3).to(DEV)
    mask = torch.randn(PE_B, 576, PE_SHAPE[0] // 8, PE_SHAPE[1] // 8, generator=g).to(DEV)
    outs = []
    for kw in ({}, {'pyramid_levels': 1}):
        L = _loss(dict(cfg, **kw))
        batch = L.order_events({'events': ev.to(DEV), 'num_pos_events': num_pos})          # (the reproducible backward)
        cg = coeff.clone().requires_grad_(True)
        l1, _, m1 = L.calc_per_event_basis(cg, 0.41, batch, 2)
        l1.backward()
        pg, mg = params.clone().requires_grad_(True), mask.clone().requires_grad_(True)
        l2, _, m2 = L.calc_per_event_curves(pg, 0.41, batch, up_mask=mg)
        l2.backward()
        outs.append((l1.detach(), cg.grad, m1['iwes'], l2.detach(), pg.grad, mg.grad, m2['iwes']))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 3. calc ---------------------------------------------------------------------------------------------------------------------
def _calc_step(L, traj, times, batch, grad=True):
    t = traj.to(DEV).requires_grad_(grad)
    loss, log, misc = L.calc(t, times.to(DEV), batch)
    if grad:
        loss.backward()
    return loss.detach().clone(), log['focus_loss'].clone(), (t.grad.clone() if grad else None), misc['iwes'].clone()


def test_calc_with_bucket_ordered_events_is_the_unordered_loss_bit_for_bit():
    import test_gpu_pyramid as TP
    cfg, ev, num_pos, traj, times = TP._case('l1', 'on_flow_to_tref')
    L = _loss(dict(cfg, pyramid_levels=3, auto_static_shapes=False))
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    a = _calc_step(L, traj, times, batch)
    b = _calc_step(L, traj, times, L.order_events(batch))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_static_shapes_replays_the_pyramid_bit_for_bit():
    import test_gpu_pyramid as TP
    cfg, ev, num_pos, traj, times = TP._case('l2', 'on_flow_to_next')
    Le = _loss(dict(cfg, pyramid_levels=3, auto_static_shapes=False))
    Ls = _loss(dict(cfg, pyramid_levels=3, static_shapes=True))
    g = torch.Generator().manual_seed(1)
    for it in range(3):
        tr = traj + 0.05 * torch.randn(traj.shape, generator=g)
        ev_i = ev.clone()
        ev_i[..., :2] += 0.01 * it * (ev[..., 5:6] != 0)
        batch = {'events': ev_i.to(DEV), 'num_pos_events': num_pos}
        a = _calc_step(Le, tr, times, batch)
        b = _calc_step(Ls, tr, times, batch)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), it
    assert len(Ls._static_plans) == 1


@pytest.mark.parametrize('norm', ['l2', 'l1'])
def test_the_stage_call_route_agrees_with_the_fused_one(norm):
    """pyramid_fused=False (ops.PyramidFocusFn) against the fused pass.  Scalars: rel 1e-6, the bound of test 1.  Gradient: both
    routes hand the SAME linear backward kernels adjoint images that differ per pixel by at most (2 L + 2) 2^-24 = 4.8e-7 of
    sum_l |r_l g_l| (test 1, L = 3); a linear map carries that into the trajectories amplified by at most the cancellation of its
    sums (sum |terms| / |sum terms|), for which a factor 20 is allowed: relative L2 below 1e-5."""
    import test_gpu_pyramid as TP
    cfg, ev, num_pos, traj, times = TP._case(norm, 'on_flow_to_tref')
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    a = _calc_step(_loss(dict(cfg, pyramid_levels=3, auto_static_shapes=False)), traj, times, batch)
    b = _calc_step(_loss(dict(cfg, pyramid_levels=3, pyramid_fused=False)), traj, times, batch)
    rel = float((a[2] - b[2]).double().norm() / b[2].double().norm())
    print(f'{norm}: loss {float(a[0]):.9g} / {float(b[0]):.9g}, focus {float(a[1]):.9g} / {float(b[1]):.9g}, gradient rel L2 {rel:.3e}')
    assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(b[0])) and abs(float(a[1]) - float(b[1])) <= 1e-6 * abs(float(b[1]))
    assert rel < 1e-5
    assert torch.equal(a[3], b[3])


# ---- 4. launch counts ------------------------------------------------------------------------------------------------------------
def _launches(L, traj, times, batch, grad):
    from motionpriorcmax_amd import ops
    t = traj.to(DEV).requires_grad_(grad)
    with ops.KernelTimer() as kf:
        loss, _, _ = L.calc(t, times.to(DEV), batch)
    kb = None
    if grad:
        with ops.KernelTimer() as kb:
            loss.backward()
    count = lambda kt: sum(r['launches'] for r in kt.summary().values())
    return count(kf), (count(kb) if grad else None), set(kf.summary()) | (set(kb.summary()) if grad else set())


def test_the_fused_pyramid_costs_three_launches():
    import test_gpu_pyramid as TP
    cfg, ev, num_pos, traj, times = TP._case('l1', 'on_flow_to_tref')
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    L1, L3 = (_loss(dict(cfg, pyramid_levels=lv, auto_static_shapes=False)) for lv in (1, 3))
    f1, b1, _ = _launches(L1, traj, times, batch, True)
    f3, b3, names = _launches(L3, traj, times, batch, True)
    print('forward launches', f1, f3, 'backward', b1, b3, sorted(names))
    assert f1 > 0 and f1 < f3 <= f1 + 3
    assert b3 == b1
    assert not [n for n in names if n.startswith('k_pool2')]
    assert {'k_iwe_pyramid_levels', 'k_iwe_pyramid_reduce', 'k_iwe_pyramid_fold'} <= names
    n1, _, _ = _launches(L1, traj, times, batch, False)
    n3, _, names = _launches(L3, traj, times, batch, False)
    assert n1 < n3 <= n1 + 2 and 'k_iwe_pyramid_fold' not in names


# ---- 5. no host synchronisation --------------------------------------------------------------------------------------------------
def test_the_pyramid_step_does_not_synchronise():
    import test_gpu_pyramid as TP
    cfg, ev, num_pos, traj, times = TP._case('l2', 'on_flow_to_tref')
    L = _loss(dict(cfg, pyramid_levels=3, auto_static_shapes=False))
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    t, tm = traj.to(DEV).requires_grad_(True), times.to(DEV)
    L.calc(t, tm, batch)[0].backward()          # (first call: module loading)
    torch.cuda.synchronize()
    t.grad = None
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss, _, _ = L.calc(t, tm, batch)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(loss).item() and torch.isfinite(t.grad).all()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_what_stays_refused_raises_before_any_launch():
    import test_gpu_pyramid as TP
    import knn_wide_cases as KC
    from motionpriorcmax_amd import ops
    from oracle import focus_oracle as O
    cfg, ev, num_pos, traj, times = TP._case('l1', 'on_flow_to_tref')
    batch = {'events': ev.to(DEV), 'num_pos_events': num_pos}
    coeff = torch.zeros(2, 1, 4, 96, 128, device=DEV)
    wide = KC.raw_trajectories(65536, 1, 5, seed=6, B=2).to(DEV)
    with ops.KernelTimer() as kt:
        with pytest.raises(ValueError, match='variance'):
            _loss(dict(cfg, pyramid_levels=2, loss_type='variance'))
        with pytest.raises(ValueError, match='num_tref'):
            _loss(dict(cfg, pyramid_levels=2, num_tref=2, scale_iwe_by_dt=False, polarity_aware_batching=False))
        L7 = _loss(dict(cfg, pyramid_levels=7, auto_static_shapes=False))
        with pytest.raises(ValueError, match='pyramid_levels=7'):
            L7.calc(traj.to(DEV), times.to(DEV), batch)
        with pytest.raises(ValueError, match='pyramid_levels=7'):
            L7.calc_per_event_basis(coeff, 0.41, batch, 2)
        with pytest.raises(ValueError, match='pyramid_levels=7'):
            _loss(dict(cfg, pyramid_levels=7, static_shapes=True)).calc(traj.to(DEV), times.to(DEV), batch)
        with pytest.raises(ValueError, match='65535'):
            _loss(dict(cfg, pyramid_levels=2, auto_static_shapes=False)).calc(wide, times.to(DEV), batch)
    assert kt.summary() == {}
