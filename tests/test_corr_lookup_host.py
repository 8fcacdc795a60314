"""The RAFT-spline correlation lookup on the host: utils.corr_pyramid and the plain-torch mirror behind utils.CorrLookup against the
g16_corr fixtures (tools/gen_golden_corr.py: the unmodified reference's CorrComputation / CorrBlockParallelMultiTarget /
BezierCurves.get_flow_from_reference / coords_grid in fp32, a float64 evaluation of the lookup's formula and the measured distance
between the two), and the host-only part of the C ABI.

Tolerance rule (shared with tests/test_gpu_corr_lookup.py, the rule of the g13 fixtures): nothing fixed in advance -- for every tensor
X the fixture holds err_X = max |X_reference_fp32 - X_fp64|; the assertion is max |X - X_fp64| <= max(4 * err_X, 2^-22 * max |X_fp64|).
Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

CASES = ['a', 'b', 'c', 'd', 'e']
MARGIN = 2.0 ** -10


def tol(g, name):
    return max(4.0 * float(g['err_' + name]), 2.0 ** -22 * float(np.abs(g[name + '64']).max()))


def maxdiff(t, ref64):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - ref64).max())


def check(label, got, bound):
    print(f'{label}: {got:.4g} (bound {bound:.4g})')
    assert got <= bound, (label, got, bound)


def lookup_of(g, device='cpu', level_grad=True):
    """(CorrLookup over the pyramid rebuilt from the fixture's feature maps, params, times as a list)."""
    from motionpriorcmax_amd import utils
    nl = [int(v) for v in g['num_levels']]
    levels, tix = utils.corr_pyramid(torch.from_numpy(g['fmap1']).to(device), torch.from_numpy(g['fmap2']).to(device), nl)
    levels = [lv.detach().requires_grad_(level_grad) for lv in levels]
    return utils.CorrLookup(levels, nl, radius=int(g['radius'])), torch.from_numpy(g['params']).to(device), [float(t) for t in g['times']]


def centres(params, times):
    """coords0 + flows, [T, B, 2, h, w]: raft.py:178-179 with the functions of this package."""
    from motionpriorcmax_amd import utils
    B, _, h, w = params.shape
    return utils.coords_grid(B, h, w, params.device, params.dtype)[None] + utils.flows_from_bezier(params, times)


def redraw_to_margin(params, times, num_levels, gen, amp):
    """The control points of every pixel where some coords / 2^l lies within 2^-10 of an integer are drawn again (CPU tensors); the
    margin is asserted.  The coordinate gradient has a kink at integers, and a fp32 coordinate is about 1e-6 off."""
    for _ in range(64):
        c = centres(params.double(), times)
        near = torch.zeros(params.shape[0], *params.shape[2:], dtype=torch.bool)
        for l in range(num_levels):
            s = c / 2 ** l
            near |= ((s - torch.round(s)).abs() < 2 * MARGIN).any(dim=2).any(dim=0)
        if not bool(near.any()):
            break
        params = torch.where(near[:, None], torch.randn(params.shape, generator=gen) * amp, params)
    c = centres(params.double(), times)
    assert min(float((c / 2 ** l - torch.round(c / 2 ** l)).abs().min()) for l in range(num_levels)) >= MARGIN
    return params


def assert_zero_where_fp64_is(t, ref64):
    z = torch.from_numpy(ref64 == 0)
    if bool(z.any()):
        assert float(t.detach().cpu()[z].abs().max()) == 0.0


def run_fixture(g, device='cpu'):
    """Both calls with every gradient; returns (out of lookup_bezier, grad_params, grad levels, out of lookup, grad_coords)."""
    lk, p, times = lookup_of(g, device)
    p.requires_grad_(True)
    go = torch.from_numpy(g['g']).to(device)
    out = lk.lookup_bezier(p, times)
    grads = torch.autograd.grad(out, [p] + lk.levels, go)
    c = centres(p.detach(), times).requires_grad_(True)
    out_c = lk.lookup(c)
    (gc,) = torch.autograd.grad(out_c, c, go)
    return out, grads[0], grads[1:], out_c, gc


def check_fixture(case, g, res):
    out, gp, gl, out_c, gc = res
    assert out.dtype == torch.float32 and out.shape == g['out64'].shape and out.is_contiguous()
    check(f'{case} out (bezier)', maxdiff(out, g['out64']), tol(g, 'out'))
    check(f'{case} out (coords)', maxdiff(out_c, g['out64']), tol(g, 'out'))
    check(f'{case} grad_params', maxdiff(gp, g['grad_params64']), tol(g, 'grad_params'))
    check(f'{case} grad_coords', maxdiff(gc, g['grad_coords64']), tol(g, 'grad_coords'))
    assert_zero_where_fp64_is(gp, g['grad_params64'])
    assert_zero_where_fp64_is(gc, g['grad_coords64'])
    assert len(gl) == int(g['num_levels'].max())
    for l, t in enumerate(gl):
        check(f'{case} grad_level_{l}', maxdiff(t, g[f'grad_level_{l}64']), tol(g, f'grad_level_{l}'))
        assert_zero_where_fp64_is(t, g[f'grad_level_{l}64'])
    for t in (out, gp, gc) + tuple(gl):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize('case', CASES)
def test_mirror_matches_the_fixtures(case):
    g = load_golden('g16_corr_' + case)
    check_fixture(case, g, run_fixture(g))


@pytest.mark.parametrize('case', CASES)
def test_pyramid_is_rebuilt_bit_for_bit(case):
    from motionpriorcmax_amd import utils
    g = load_golden('g16_corr_' + case)
    nl = [int(v) for v in g['num_levels']]
    levels, tix = utils.corr_pyramid(torch.from_numpy(g['fmap1']), torch.from_numpy(g['fmap2']), nl)
    assert len(levels) == max(nl) == len(tix)
    B, D, h, w = g['fmap1'].shape
    for l, lv in enumerate(levels):
        assert lv.dtype == torch.float32 and tuple(lv.shape) == (len(tix[l]), B * h * w, 1, h >> l, w >> l)
        assert hashlib.sha256(lv.contiguous().numpy().tobytes()).digest() == g[f'level_sha_{l}'].tobytes()
        assert tix[l] == g[f'target_indices_{l}'].tolist() and all(isinstance(t, int) for t in tix[l])
    assert tix == utils.level_target_indices(nl)


def test_lookup_of_the_curve_centres_equals_lookup_bezier():
    g = load_golden('g16_corr_c')
    lk, p, times = lookup_of(g, level_grad=False)
    a = lk.lookup_bezier(p, times)
    assert torch.equal(a, lk.lookup(centres(p, times)))
    assert torch.equal(a, lk.lookup_bezier(p, torch.tensor(times, dtype=torch.float64)))
    assert torch.equal(a, lk(centres(p, times)))


def test_a_list_behaves_as_the_stacked_tensor():
    g = load_golden('g16_corr_b')
    lk, p, times = lookup_of(g, level_grad=False)
    c = centres(p, times)
    assert torch.equal(lk.lookup(list(c.unbind(0))), lk.lookup(c))
    assert torch.equal(lk.lookup(tuple(c.unbind(0))), lk.lookup(c))
    with pytest.raises(ValueError):
        lk.lookup(c[:2])
    with pytest.raises(ValueError):
        lk.lookup_bezier(p, times[:2])


def test_from_block_reads_a_duck_typed_pyramid():
    from motionpriorcmax_amd import utils

    class Data:
        def __init__(self, corr, tix):
            self.corr, self.target_indices = corr, torch.tensor(tix)

    class Block:
        pass

    g = load_golden('g16_corr_c')
    lk, p, times = lookup_of(g, level_grad=False)
    block = Block()
    block._corr_pyramid = [Data(lv, t) for lv, t in zip(lk.levels, lk.target_indices)]
    block._radius = 4
    want = lk.lookup_bezier(p, times)
    for nl in ([2, 1], None):
        got = utils.CorrLookup.from_block(block, nl)
        assert got.target_indices == [[0, 1], [0]] and got.num_levels_per_target == [2, 1] and got.radius == 4
        assert torch.equal(got.lookup_bezier(p, times), want)


def test_a_degenerate_level_raises():
    from motionpriorcmax_amd import utils
    f1, f2 = torch.zeros(1, 4, 3, 4), torch.zeros(1, 1, 4, 3, 4)
    levels, _ = utils.corr_pyramid(f1, f2, [2])                   # level 1 is 1 x 2
    with pytest.raises(ValueError, match='2 x 2'):
        utils.CorrLookup(levels, [2])
    utils.CorrLookup(levels[:1], [1])
    with pytest.raises(ValueError):
        utils.CorrLookup(levels[:1], [2])                         # a level is missing


def test_header_declares_and_library_exports_the_entry_points():
    from motionpriorcmax_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mpc_corr_lookup_supported', 'mpc_corr_lookup_fwd', 'mpc_corr_lookup_bwd'):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    macros = {m: int(v) for m, v in re.findall(r'#define (MPC_CORR_[A-Z_]+) (\d+)', header)}
    assert (macros['MPC_CORR_MAX_LEVELS'], macros['MPC_CORR_MAX_TARGETS'], macros['MPC_CORR_MAX_RADIUS'], macros['MPC_CORR_F_LANE_PER_QUERY']) == \
        (_lib.CORR_MAX_LEVELS, _lib.CORR_MAX_TARGETS, _lib.CORR_MAX_RADIUS, _lib.CORR_F_LANE_PER_QUERY)
    assert _lib.lib().mpc_version() == 107


def descriptor(h=48, w=64, num_levels=(1, 1, 1, 1, 4), radius=4, d=10, B=2):
    """A descriptor without device memory (host-only checks)."""
    from motionpriorcmax_amd import _lib, utils
    tix = utils.level_target_indices(list(num_levels))
    desc = _lib.CorrDesc(B=B, h=h, w=w, T=len(num_levels), d=d, radius=radius, num_levels=len(tix))
    for l, ts in enumerate(tix[:_lib.CORR_MAX_LEVELS]):
        desc.level_h[l], desc.level_w[l], desc.level_n[l] = h >> l, w >> l, len(ts)
        for s, t in enumerate(ts[:_lib.CORR_MAX_TARGETS]):
            desc.level_target[l][s] = t
    return desc


def test_supported_reports_the_limits_on_the_host():
    from motionpriorcmax_amd import _lib
    L = _lib.lib()

    def rc(desc):
        return L.mpc_corr_lookup_supported(ctypes.byref(desc))
    assert rc(descriptor()) == 0
    assert rc(descriptor(radius=1, d=16, num_levels=[1] * 16)) == 0 and rc(descriptor(h=64, w=64, num_levels=[6])) == 0
    assert rc(descriptor(radius=5)) == _lib.E_UNSUPPORTED
    assert b'radius' in L.mpc_last_error_string()
    assert rc(descriptor(d=17)) == _lib.E_UNSUPPORTED
    assert rc(descriptor(num_levels=[1] * 17)) == _lib.E_UNSUPPORTED
    assert rc(descriptor(h=256, w=256, num_levels=[7])) == _lib.E_UNSUPPORTED
    assert rc(descriptor(radius=0)) == _lib.E_SHAPE
    bad = descriptor()
    bad.level_h[1] = 25                                           # 48 >> 1 is 24
    assert rc(bad) == _lib.E_SHAPE
    bad = descriptor()
    bad.level_w[3] = 7
    assert rc(bad) == _lib.E_SHAPE
    assert rc(descriptor(h=6, w=8, num_levels=[3])) == _lib.E_SHAPE       # level 2 is 1 x 2
    assert b'2 x 2' in L.mpc_last_error_string()
    bad = descriptor()
    bad.level_target[0][1] = 0                                    # not ascending
    assert rc(bad) == _lib.E_SHAPE
    assert L.mpc_corr_lookup_supported(None) == _lib.E_NULL
    assert L.mpc_corr_lookup_fwd(None, None, None, None, None, None) == _lib.E_NULL
    assert L.mpc_corr_lookup_fwd(ctypes.byref(descriptor(radius=5)), None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.mpc_corr_lookup_bwd(ctypes.byref(descriptor(d=17)), None, None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.mpc_corr_lookup_fwd(ctypes.byref(descriptor()), None, None, None, None, None) == _lib.E_NULL      # neither coords nor params


def test_cpu_tensors_and_unsupported_shapes_take_the_mirror():
    """CPU tensors never reach the library; neither does radius 5 (the routing rule of utils/corr.py)."""
    from motionpriorcmax_amd import utils
    g = load_golden('g16_corr_a')
    lk, p, times = lookup_of(g, level_grad=False)
    assert not lk._kernels_serve(p, 3)
    wide = utils.CorrLookup(lk.levels, lk.num_levels_per_target, radius=5)
    out = wide.lookup_bezier(p, times)
    assert out.shape == (2, 3 * 121, 6, 8) and torch.isfinite(out).all()
