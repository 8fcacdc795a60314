"""The event kernels (csrc/events.hip) element by element against the float64 reference of tests/event_cases.py, through the stage
entry points of ops.py: k_ev_bin -> k_iwe_accum (float and Q33.30 output), k_lut_accum from the forward's records and from
bucket-ordered rows with the offsets table, each with and without add_term, the global-atomic kernels (atomic_path, and num_tref = 3
as it comes), and the imager path ops.splat_events (MPC_F_NO_WARP, with and without MPC_F_UNIT_WEIGHT).

Every bound is the running error bound derived in tests/event_cases.py from the roundings counted in the kernels; no element is
excused, and an element with allowance zero must be exactly zero.  Random LUT of a few pixels, random adjoint image and add_term,
GCOEF and grad_out not 1, a workspace of its own per call.  The figures are printed before they are asserted (pytest -s);
profiles/event_cases_runs.md has those of an MI355X.

Three switches of the layout are read once per process (api.hip: mpc_layout); for each, a selection of this file runs again in a
fresh interpreter: MPC_EV_EXACT_ABOVE_MB=0 (exact-size backward buckets: k_ev_count / k_ev_prefix), MPC_EV_STRIPS=48 (one-row image
strips: every vote straddles a seam and a k_ev_bin workgroup has more records than its staging area holds, the direct-emit branch)
and MPC_EV_CSTRIP_KB=64 (LUT strips with more cells than k_lut_accum prefetches of add_term: its un-prefetched tail).

Measured on an MI355X: every tiled and ordered figure equals the host stand-in's (integer sums); the largest ratios are 0.9996 forward
(a seam tap of weight 2^-20 whose truncation is nearly the whole allowance of its pixel), 0.97 backward, 0.99 with add_term (cells that
hold grad_out * add_term alone), 0.50 for the atomic kernels.  67 tests in 15 s, 13 of them in the three child interpreters."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_cases as E

pytestmark = pytest.mark.gpu

LUT_ADD_PF_CELLS = 6 * 512          # csrc/tuning.h: EV_LUT_ADD_PF * EV_LUT_THREADS


def _dev():
    return torch.device('cuda:0')


def _cfg(c, atomic=False):
    from motionpriorcmax_amd import ops
    return ops.PathConfig(image_shape=(c.H, c.W), num_tref=c.T, num_bins=c.nb, num_knn=0, smooth_weight=0.0, sp=c.sp, norm_l2=False,
                          dist_l1=False, scale_by_dt=c.scale_dt, mask_border=c.mask, polarity_split=c.split, scheme_iwd=False,
                          smooth_on_next=False, atomic_path=atomic)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stages(c, cfg, ev, offs=None, fixed=True):
    """mpc_event_splat_fwd (and _fixed), then mpc_event_splat_bwd without and with add_term, each call on a workspace of its own (the
    backward on the forward's: it reads the records left there) -> raw, fixed, g0, g1, kernels seen."""
    from motionpriorcmax_amd import _lib as C, ops
    dev = _dev()
    shape = ops.make_shape(cfg, c.B, c.M, c.num_pos, 0, K=0)
    lut, t_ref, gimg, add = _t(c.lut), _t(c.t_ref), _t(c.gimg), _t(c.add)
    scal = torch.ones(C.SCAL_COUNT, device=dev)
    scal[C.SCAL_GCOEF] = E.GCOEF
    gout = torch.tensor([E.GOUT], device=dev)
    with ops.KernelTimer() as kt:
        fx = ops.event_splat_fwd_fixed(shape, ev, lut, t_ref, ops.alloc_workspace(shape, dev)) if fixed else None
        out = []
        for a in (None, add):
            ws = ops.alloc_workspace(shape, dev)
            raw = ops.event_splat_fwd(shape, ev, lut, t_ref, ws)
            out.append(ops.event_splat_bwd(shape, ev, lut, t_ref, gimg, scal, gout, torch.empty_like(lut), a, ws, offs))
    return raw.cpu().numpy(), None if fx is None else fx.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy(), set(kt.summary()), shape


def _check_all(name, path, c, raw, fx, g0, g1, atomic=False):
    f = E.reference_fwd(c) if c is not E.case(name) else E.expected_fwd(name)
    b0, b1 = (E.reference_bwd(c, add=a) if c is not E.case(name) else E.expected_bwd(name, a) for a in (False, True))
    key = 'allow_atomic' if atomic else 'allow'
    E.check(name, f'{path} fwd', raw, f['ref'], f[key], c, f['prov'])
    if fx is not None:
        E.check(name, f'{path} fwd fixed', fx.astype(np.float64) * E.Q30, f['ref'], f['allow_fixed'], c, f['prov'])
    E.check(name, f'{path} bwd', g0, b0['ref'], b0[key], c, b0['prov'])
    E.check(name, f'{path} bwd add_term', g1, b1['ref'], b1[key], c, b1['prov'])


@pytest.mark.parametrize('name', E.T1_CASES)
def test_tiled_forward_and_record_backward(name):
    from motionpriorcmax_amd import ops
    c = E.case(name)
    raw, fx, g0, g1, seen, shape = _stages(c, _cfg(c), _t(c.ev))
    assert {'k_ev_bin', 'k_iwe_accum', 'k_lut_accum'} <= seen and not any('atomic' in k for k in seen), seen
    if os.environ.get('MPC_EV_EXACT_ABOVE_MB') == '0':
        assert {'k_ev_count', 'k_ev_prefix'} <= seen, seen
    if name.startswith('lut_seams'):
        ncs = ops._lut_strips(shape, _dev())
        assert ncs >= 2, ncs
        if os.environ.get('MPC_EV_CSTRIP_KB') == '64' and name == 'lut_seams_tall':
            assert -(-shape.hq // ncs) * shape.wq > LUT_ADD_PF_CELLS, (ncs, shape.hq, shape.wq)
    _check_all(name, 'tiled', c, raw, fx, g0, g1)


@pytest.mark.parametrize('name', E.T1_CASES)
def test_bucket_ordered_rows_and_ordered_backward(name):
    """ops.event_bucket_order permutes the rows inside a polarity block: the reference is built from the ordered tensor."""
    from motionpriorcmax_amd import ops
    c = E.case(name)
    cfg = _cfg(c)
    evo, offs = ops.event_bucket_order(cfg, _t(c.ev), c.num_pos)
    o = c.with_events(evo.cpu().numpy())
    o.kind, o.kinds = (o.ev[..., 5] != 0).astype(np.int64), ['pad', 'ordered_row']
    for b in range(c.B):            # the same rows, sample by sample
        assert sorted(map(tuple, o.ev[b].tolist())) == sorted(map(tuple, c.ev[b].tolist()))
    raw, _, g0, g1, seen, _ = _stages(o, cfg, evo, offs=offs, fixed=False)
    assert {'k_ev_bin', 'k_iwe_accum', 'k_lut_accum'} <= seen, seen
    _check_all(name, 'ordered', o, raw, None, g0, g1)
    # far rows and rows the mask drops give exact zeros: cells without a contribution hold nothing (no add_term)
    assert bool((g0[E.reference_bwd(o, add=False)['n'] == 0] == 0).all())


@pytest.mark.parametrize('name', E.T1_CASES + ('num_tref_3',))
def test_global_atomic_kernels(name):
    c = E.case(name)
    raw, _, g0, g1, seen, _ = _stages(c, _cfg(c, atomic=(c.T == 1)), _t(c.ev), fixed=False)
    assert {'k_splat_fwd_atomic', 'k_splat_bwd_atomic'} <= seen and not ({'k_ev_bin', 'k_lut_accum'} & seen), seen
    _check_all(name, 'atomic', c, raw, None, g0, g1, atomic=True)


@pytest.mark.parametrize('unit', [False, True])
@pytest.mark.parametrize('name', E.SPLAT_CASES)
def test_imager_path_without_warp(name, unit):
    from motionpriorcmax_amd import ops
    s = E.splat_rows(name)
    f = E.reference_fwd(s, no_warp=True, unit_weight=unit)
    with ops.KernelTimer() as kt:
        img = ops.splat_events((s.H, s.W), _t(s.ev), unit, False)
    assert {'k_ev_bin', 'k_iwe_accum'} <= set(kt.summary()), set(kt.summary())
    E.check(name, f'splat_events unit_weight={unit}', img.cpu().numpy(), f['ref'], f['allow'], s, f['prov'])


def _child(env, sel):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', 'tests/test_gpu_event_cases.py', '-x', '-q', '-s', '-m', 'gpu', '-k', sel],
                       cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    print('\n'.join(f'{env}: {line}' for line in r.stdout.splitlines() if ' ratio ' in line), flush=True)
    assert r.returncode == 0 and ' passed' in r.stdout and 'skipped' not in r.stdout, (r.stdout[-2500:], r.stderr[-500:])


def test_exact_size_buckets_in_a_child_process():
    """MPC_EV_EXACT_ABOVE_MB=0: the backward buckets are sized by the counting pass and lie back to back in the sample's region."""
    _child({'MPC_EV_EXACT_ABOVE_MB': '0'}, 'test_tiled and (lut_seams or clamped_cells)')


def test_one_row_image_strips_in_a_child_process():
    """MPC_EV_STRIPS=48 on the 48-row cases: every vote straddles a seam, and the first k_ev_bin workgroup of rows_and_columns has
    more than EV_STAGE records (tests/test_event_cases_host.py counts them): the direct-emit branch."""
    _child({'MPC_EV_STRIPS': '48'}, '(test_tiled or test_bucket_ordered or test_imager) and (rows_and_columns or below_integer)')


def test_lut_strips_beyond_the_add_term_prefetch_in_a_child_process():
    """MPC_EV_CSTRIP_KB=64: lut_seams_tall has two LUT strips of 40 x 96 = 3 840 cells, more than the 3 072 whose add_term a
    k_lut_accum workgroup requests at its top, so the un-prefetched tail writes the rest (64 x 96 gives exactly 3 072: no tail)."""
    _child({'MPC_EV_CSTRIP_KB': '64'}, 'test_tiled and lut_seams')
