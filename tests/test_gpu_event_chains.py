"""The two LDS-accumulate kernels of the event path request their first records before they know the bucket's count
(k_iwe_accum: 1024 threads x 4 records, k_lut_accum: 512 x 4; events.hip): the index of those loads is clamped to the
bucket's capacity, and what comes back from beyond the count is dropped before anything is derived from it.  The
stage entry points are driven here with a zero-flow LUT and events placed so that ONE forward bucket and ONE backward
bucket receive exactly n records and every other bucket none, n at the edges of that load pattern.

Every case is compared with the CPU oracle at the tolerances of tests/test_gpu_parity.py for the same stage outputs
(raw IWE: atol 1e-5 * max, d/dLUT: relative L2 1e-4), element by element with the float64 reference of tests/event_cases.py under its
counted rounding bound, and bit for bit between two runs and between the time-ordered
and the bucket-ordered layout of the same events (integer accumulators: no order dependence)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_cases as E

pytestmark = pytest.mark.gpu

IMG, SP, NB, B = (160, 640), 4, 3, 2
T_REF = 0.41
GCOEF, GOUT = 1.25, 0.75             # (their product is exact in fp32)
LUT_NT, IWE_NT, NIF = 512, 1024, 4
EDGES = sorted({n for nt in (LUT_NT, IWE_NT) for n in (0, 1, nt - 1, nt, nt + 1, NIF * nt - 1, NIF * nt, NIF * nt + 1, 2 * NIF * nt + 3)})


def _cfg(split=True):
    return dict(image_shape=IMG, num_tref=1, num_bins=NB, num_knn=4, smooth_weight=0.0, lut_superpixel_size=SP,
                focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True,
                polarity_aware_batching=split, interpolation_scheme='mean', smooth_type='on_flow_to_tref')


def _events(n, M, num_pos, split, sample, seed):
    """[B, M, 6] rows (y, x, t, p, bin, valid): n live rows of `sample`, all in image rows 2..6 (one image strip, LUT rows 0..1: one
    LUT strip), time bin 1 and ONE polarity block (the second, unless it is empty); every other row is a zero row -- no record."""
    g = torch.Generator().manual_seed(seed)
    ev = torch.zeros(B, M, 6)
    lo, hi = (num_pos, M) if (split and num_pos < M) else (0, M)
    assert n <= hi - lo
    rows = lo + torch.randperm(hi - lo, generator=g)[:n]
    r = torch.rand(n, 3, generator=g)
    ev[sample, rows, 0] = 2.25 + 3.5 * r[:, 0]
    ev[sample, rows, 1] = 0.5 + (IMG[1] - 2.0) * r[:, 1]
    ev[sample, rows, 2] = 0.3 + 0.2 * r[:, 2]
    ev[sample, rows, 3] = 1.0
    ev[sample, rows, 4] = 1.0
    ev[sample, rows, 5] = 1.0
    return ev


def _stages(L, ev, num_pos, gimg, add, offs=None, ws_fill=None, forward=True):
    """mpc_event_splat_fwd, then mpc_event_splat_bwd without and with add_term, on a workspace of their own."""
    from motionpriorcmax_amd import _lib as C, ops
    dev = ev.device
    cfg = L._cfg
    M = ev.shape[1]
    shape = ops.make_shape(cfg, B, M, num_pos if cfg.polarity_split else M, 0, K=0)
    ws = ops.alloc_workspace(shape, dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    hq, wq = cfg.lut_grid
    lut = torch.zeros(B, NB, hq, wq, 1, 2, device=dev)
    t_ref = torch.tensor([T_REF], device=dev)
    raw = ops.event_splat_fwd(shape, ev, lut, t_ref, ws) if forward else None
    scal = torch.ones(C.SCAL_COUNT, device=dev)
    scal[C.SCAL_GCOEF] = GCOEF
    gout = torch.tensor([GOUT], device=dev)
    g0 = ops.event_splat_bwd(shape, ev, lut, t_ref, gimg, scal, gout, torch.empty_like(lut), None, ws, offs)
    g1 = ops.event_splat_bwd(shape, ev, lut, t_ref, gimg, scal, gout, torch.empty_like(lut), add, ws, offs)
    return raw, g0, g1


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


def _check(n, M, num_pos, split=True, sample=0):
    from motionpriorcmax_amd import LossFactory, ops
    from oracle import focus_oracle as O
    dev = torch.device('cuda:0')
    cfg = _cfg(split)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    ev = _events(n, M, num_pos, split, sample, seed=1000 + n)
    g = torch.Generator().manual_seed(7)
    P = 2 if split else 1
    gimg = torch.randn(B, P, *IMG, generator=g)
    hq, wq = L._cfg.lut_grid
    add = torch.randn(B, NB, hq, wq, 1, 2, generator=g)
    # CPU oracle: the raw image, and d/dLUT of <raw, gimg>
    lo = torch.zeros(B, NB, hq, wq, 1, 2, requires_grad=True)
    _, _, rawo = O.FocusLossOracle(**cfg).event_path(ev, lo, torch.tensor([T_REF]), num_pos)
    (rawo.reshape(gimg.shape) * gimg).sum().backward()
    want = (GCOEF * GOUT) * lo.grad
    evd, gd, ad = ev.to(dev), gimg.to(dev), add.to(dev)
    raw, g0, g1 = _stages(L, evd, num_pos, gd, ad)
    live = ev[..., 5] != 0
    assert int(live.sum()) == n
    mass = float((1.0 - (ev[..., 2][live] - T_REF).abs()).double().sum())      # every live row votes with all four taps
    assert abs(float(rawo.detach().double().sum()) - mass) <= 1e-4 * max(mass, 1.0)
    np.testing.assert_allclose(raw.cpu().numpy().reshape(rawo.shape), rawo.detach().numpy(), rtol=0,
                               atol=1e-5 * max(1.0, float(rawo.max())))
    err = _rel_l2(g0.cpu().numpy(), want.numpy())
    print(f'n {n} M {M} num_pos {num_pos} split {split}: d/dLUT rel L2 {err:.3e}')
    assert err < 1e-4
    # every element against the float64 reference, under the bound counted from the kernels' roundings (tests/event_cases.py)
    c = E.Case(name='chain', H=IMG[0], W=IMG[1], sp=SP, nb=NB, T=1, B=B, split=split, scale_dt=True, mask=True,
               num_pos=num_pos if split else M, ev=ev.numpy(), kind=(ev[..., 5] != 0).long().numpy(), kinds=['pad', 'live'],
               lut=np.zeros((B, NB, hq, wq, 1, 2), dtype=np.float32), gimg=gimg.numpy(), add=add.numpy(),
               t_ref=np.array([T_REF], dtype=np.float32))
    f = E.reference_fwd(c)
    E.check(f'n {n} M {M}', 'fwd', raw.cpu().numpy(), f['ref'], f['allow'], c, f['prov'])
    for with_add, got in ((False, g0), (True, g1)):
        r = E.reference_bwd(c, add=with_add, gcoef=GCOEF, gout=GOUT)
        E.check(f'n {n} M {M}', f'bwd add_term={with_add}', got.cpu().numpy(), r['ref'], r['allow'], c, r['prov'])
    # add_term: one product and one sum per element on top of the same value (no contraction in either place)
    assert torch.equal(g1, g0 + GOUT * ad)
    # two runs
    raw_b, g0_b, g1_b = _stages(L, evd, num_pos, gd, ad)
    assert torch.equal(raw_b, raw) and torch.equal(g0_b, g0) and torch.equal(g1_b, g1)
    # bucket-ordered rows of the same events: the backward reads the event rows through the offsets table
    evo, offs = ops.event_bucket_order(L._cfg, evd, num_pos)
    raw_o, g0_o, g1_o = _stages(L, evo, num_pos, gd, ad, offs=offs)
    assert torch.equal(raw_o, raw) and torch.equal(g0_o, g0) and torch.equal(g1_o, g1)


@pytest.mark.parametrize('n', EDGES)
def test_bucket_fill_at_the_edges_of_the_load_pattern(n):
    """M = n + 37 rows, the second polarity block holds the live rows; up to n = 2011 the capacity of the bucket (M) lies
    below the 2 048 records a k_lut_accum workgroup asks for ahead of the count, so the capacity clamp bounds the loads."""
    _check(n, n + 37, 5)


@pytest.mark.parametrize('n,M,num_pos', [(513, 513, 0), (513, 513, 513), (300, 700, 350), (1500, 1500, 0)])
def test_capacity_below_the_loads_in_flight_and_empty_polarity_blocks(n, M, num_pos):
    """Buckets filled to their last slot (M = n), M below NIF * NT for both kernels, and a polarity block without rows
    (num_pos = 0 and num_pos = M: the capacity of the forward buckets is the other block's)."""
    _check(n, M, num_pos)


@pytest.mark.parametrize('n', [1, 513, 2049])
def test_one_polarity_records_only_in_the_last_sample(n):
    """polarity_aware_batching off: one image per sample, and the live records belong to the LAST sample -- a polarity bit
    taken from a record beyond the count would select an image behind the last one of the adjoint tensor."""
    _check(n, n + 37, n + 37, split=False, sample=B - 1)


@pytest.mark.parametrize('fill', [0, 0xA5])
def test_backward_without_forward_records_gives_nan(fill):
    """A workspace the forward never wrote records (and their marker) into: the coefficient is NaN and so is every
    element of d/dLUT, with or without add_term, whatever the counters hold."""
    from motionpriorcmax_amd import LossFactory
    dev = torch.device('cuda:0')
    L = LossFactory.get_loss_calculator('FOCUS', _cfg())
    ev = _events(700, 737, 5, True, 0, seed=3).to(dev)
    g = torch.Generator().manual_seed(7)
    gimg = torch.randn(B, 2, *IMG, generator=g).to(dev)
    hq, wq = L._cfg.lut_grid
    add = torch.randn(B, NB, hq, wq, 1, 2, generator=g).to(dev)
    _, g0, g1 = _stages(L, ev, 5, gimg, add, ws_fill=fill, forward=False)
    assert torch.isnan(g0).all().item() and torch.isnan(g1).all().item()


def test_exact_size_buckets_in_a_child_process():
    """MPC_EV_EXACT_ABOVE_MB is read once per process: with 0 the backward buckets are sized by the counting pass and lie
    back to back in the sample's region (the records asked for ahead of the count are clamped to the end of that
    region).  Some of the cases above (never this one) are run again in a fresh interpreter with the switch set."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sel = 'edges_of_the_load_pattern and (2049 or 511) or capacity_below and 513-513-0 or backward_without_forward'
    r = subprocess.run([sys.executable, '-m', 'pytest', 'tests/test_gpu_event_chains.py', '-x', '-q', '-m', 'gpu', '-k', sel],
                       cwd=root, env=dict(os.environ, MPC_EV_EXACT_ABOVE_MB='0'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ' passed' in r.stdout and 'skipped' not in r.stdout, (r.stdout[-1500:], r.stderr[-500:])
