"""The fused RAFT-spline correlation pyramid on the host: the C ABI's host-only part (include/mpcmax.h: mpc_corr_pyramid_*), and the
routing of utils.corr_pyramid_fused / CorrLookup.from_fmaps for tensors the kernels do not take -- they must be `corr_pyramid` itself,
bit for bit, errors included."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from test_corr_lookup_host import CASES, descriptor

NAMES = ('mpc_corr_pyramid_workspace_bytes', 'mpc_corr_pyramid_supported', 'mpc_corr_pyramid_fwd', 'mpc_corr_pyramid_bwd')


def test_header_declares_and_library_exports_the_entry_points():
    from motionpriorcmax_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert _lib.lib().mpc_version() == 107
    assert re.search(r'#define MPC_VERSION 107\b', header)


def test_supported_reports_the_limits_on_the_host():
    from motionpriorcmax_amd import _lib
    L = _lib.lib()

    def rc(desc, D):
        return L.mpc_corr_pyramid_supported(ctypes.byref(desc), D)
    assert rc(descriptor(), 256) == 0 and rc(descriptor(), 4) == 0 and rc(descriptor(), 512) == 0
    assert rc(descriptor(h=6, w=8, num_levels=[3]), 16) == 0              # a 1 x 2 level is a pyramid level (the lookup refuses it)
    assert rc(descriptor(num_levels=[1] * 16), 256) == 0 and rc(descriptor(h=64, w=64, num_levels=[6]), 8) == 0
    assert rc(descriptor(), 6) == _lib.E_UNSUPPORTED
    assert b'multiple of 4' in L.mpc_last_error_string()
    assert rc(descriptor(), 516) == _lib.E_UNSUPPORTED
    assert rc(descriptor(h=256, w=256, num_levels=[7]), 256) == _lib.E_UNSUPPORTED
    assert rc(descriptor(num_levels=[1] * 17), 256) == _lib.E_UNSUPPORTED
    bad = descriptor(num_levels=[3, 2, 1])
    bad.level_target[2][0] = 2                                            # level 2 = {2}, level 1 = {0, 1}: not nested
    assert rc(bad, 256) == _lib.E_SHAPE
    bad = descriptor()
    bad.level_target[0][1] = 0                                            # not ascending
    assert rc(bad, 256) == _lib.E_SHAPE
    bad = descriptor()
    bad.level_h[1] = 25
    assert rc(bad, 256) == _lib.E_SHAPE
    assert rc(descriptor(h=2, w=8, num_levels=[3]), 16) == _lib.E_SHAPE   # level 2 is 0 x 2
    assert rc(descriptor(), 0) == _lib.E_SHAPE
    assert L.mpc_corr_pyramid_supported(None, 256) == _lib.E_NULL
    assert L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(descriptor()), 6, 0) == _lib.E_UNSUPPORTED
    assert L.mpc_corr_pyramid_fwd(ctypes.byref(descriptor()), 516, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.mpc_corr_pyramid_bwd(ctypes.byref(descriptor()), 6, None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.mpc_corr_pyramid_fwd(ctypes.byref(descriptor()), 256, None, None, None, None) == _lib.E_NULL
    assert L.mpc_corr_pyramid_fwd(ctypes.byref(descriptor(B=0)), 256, None, None, None, None) == 0


def test_workspace_sizes():
    """Forward: the pooled feature maps of the levels >= 1 (rows padded to 4 floats).  Backward: those, the per-level feature-map
    gradients and the split-k partials of grad_fmap1 -- and never a volume."""
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    B, D = 6, 256
    d = descriptor(B=B)                                                   # 48 x 64, [1, 1, 1, 1, 4]
    pooled = B * D * (24 * 32 + 12 * 16 + 6 * 8) * 4
    assert L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(d), D, 0) == pooled
    bwd = L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(d), D, 1)
    gp = B * D * (5 * 48 * 64 + 24 * 32 + 12 * 16 + 6 * 8) * 4
    level0 = 5 * B * (48 * 64) ** 2 * 4
    assert pooled + gp <= bwd <= pooled + gp + 16 * B * D * 48 * 64 * 4 and bwd < level0 // 4
    assert L.mpc_corr_pyramid_workspace_bytes(ctypes.byref(descriptor(B=0)), D, 1) == 16


@pytest.mark.parametrize('case', CASES)
def test_cpu_tensors_take_corr_pyramid_bit_for_bit(case):
    from motionpriorcmax_amd import utils
    g = load_golden('g16_corr_' + case)
    nl = [int(v) for v in g['num_levels']]
    f1, f2 = torch.from_numpy(g['fmap1']), torch.from_numpy(g['fmap2'])
    want, wtix = utils.corr_pyramid(f1, f2, nl)
    got, tix = utils.corr_pyramid_fused(f1, f2, nl)
    assert tix == wtix and len(got) == len(want)
    assert all(torch.equal(a, b) and a.shape == b.shape for a, b in zip(got, want))
    if min(want[-1].shape[-2:]) >= 2:
        lk = utils.CorrLookup.from_fmaps(f1, f2, nl, radius=int(g['radius']))
        assert lk.radius == int(g['radius']) and lk.target_indices == wtix
        assert all(torch.equal(a, b) for a, b in zip(lk.levels, want))
        p, times = torch.from_numpy(g['params']), [float(t) for t in g['times']]
        assert torch.equal(lk.lookup_bezier(p, times), utils.CorrLookup(want, nl, radius=int(g['radius'])).lookup_bezier(p, times))


def test_other_inputs_take_corr_pyramid():
    from motionpriorcmax_amd import utils
    gen = torch.Generator().manual_seed(7)
    f1, f2 = torch.randn(1, 6, 4, 5, generator=gen), torch.randn(1, 6, 4, 5, generator=gen)          # one target as 4 dimensions
    want, wtix = utils.corr_pyramid(f1, f2, 2)
    got, tix = utils.corr_pyramid_fused(f1, f2, 2)
    assert tix == wtix == [[0], [0]] and all(torch.equal(a, b) for a, b in zip(got, want))
    got64, _ = utils.corr_pyramid_fused(f1.double(), f2.double(), [2])
    assert got64[0].dtype == torch.float64 and got64[1].shape == (1, 20, 1, 2, 2)
    f1.requires_grad_(True)
    levels, _ = utils.corr_pyramid_fused(f1, f2, [2])
    (ga,) = torch.autograd.grad(levels[1].sum(), f1)
    levels, _ = utils.corr_pyramid(f1, f2, [2])
    (gb,) = torch.autograd.grad(levels[1].sum(), f1)
    assert torch.equal(ga, gb)


@pytest.mark.parametrize('args', [
    (torch.zeros(1, 4, 3, 4), torch.zeros(2, 1, 4, 3, 4), [1]),                     # two targets, one level count
    (torch.zeros(1, 4, 3, 4), torch.zeros(1, 1, 4, 3, 5), [1]),                     # grids differ
    (torch.zeros(2, 4, 3, 4), torch.zeros(1, 1, 4, 3, 4), [1]),                     # batches differ
    (torch.zeros(1, 4, 3, 4), torch.zeros(1, 1, 4, 3, 4), [0]),                     # no level
    (torch.zeros(1, 4, 3, 4), torch.zeros(1, 1, 4, 3, 4), []),
])
def test_the_value_errors_are_those_of_corr_pyramid(args):
    from motionpriorcmax_amd import utils
    with pytest.raises(ValueError) as want:
        utils.corr_pyramid(*args)
    with pytest.raises(ValueError) as got:
        utils.corr_pyramid_fused(*args)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:
        utils.CorrLookup.from_fmaps(*args)
    assert str(got.value) == str(want.value)
