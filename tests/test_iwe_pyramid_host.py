"""CPU-only checks of the fused IWE pyramid pass (csrc/iwe_pyramid.hip): the float64 definition the GPU tests hold it to agrees
with the oracle chain of tests/test_gpu_pyramid.py, the three entry points are exported, the host-only support query refuses what
the header says it refuses, and the workspace grows with the levels."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import iwe_pyramid_cases as PY


def _shape(**kw):
    from motionpriorcmax_amd import _lib
    d = dict(B=2, M=0, Mp=0, nb=1, T=1, H=96, W=128, sp=4, hq=24, wq=32, n=0, K=0, flags=0)
    d.update(kw)
    return _lib.Shape(**d)


@pytest.mark.parametrize('norm', ['l1', 'l2'])
def test_the_float64_definition_is_the_oracle_chain(norm):
    from oracle import focus_oracle as O
    raw = PY.raw_images('b')
    levels = PY.CASES['b']['levels']
    d = PY.definition64(raw, levels, norm)
    r = raw.double()[:, None].clone().requires_grad_(True)
    cur, vals = r, []
    for _ in range(levels):
        vals.append(O.contrast_value(O.gaussian_blur3(cur), 'gradient_magnitude', norm))
        cur = F.avg_pool2d(cur, 2)
    focus = sum(1 / v for v in vals)
    (g,) = torch.autograd.grad(focus, r)
    assert torch.allclose(torch.stack(vals).detach(), d['vals'], rtol=1e-12, atol=0)
    assert abs(float(focus.detach()) - float(d['focus'])) <= 1e-12 * abs(float(focus.detach()))
    assert (g[:, 0] - d['grad']).abs().max() <= 1e-12 * g.abs().max()


def test_the_seeded_cases_leave_the_l1_check_its_pixels():
    """The 'l1' fold check runs outside grad_accounting.pyramid_near_zero_pixels: the chosen seeds mask less than 2 %."""
    from grad_accounting import pyramid_near_zero_pixels
    for name, c in PY.CASES.items():
        if 'seed' not in c:
            continue
        aff = pyramid_near_zero_pixels(PY.raw_images(name)[:, None], c['levels'])
        share = float(aff.float().mean())
        print(f'case {name}: masked share {share:.4f}')
        assert share < PY.MASKED_SHARE_MAX, (name, share)


def test_the_three_symbols_are_exported():
    from motionpriorcmax_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ('mpc_iwe_pyramid_supported', 'mpc_iwe_pyramid_workspace_bytes', 'mpc_iwe_pyramid_fwd'):
        assert hasattr(L, n) and n in _lib.EXPORTS, n


def test_supported_refuses_without_a_device():
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    ok = _shape()
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(ok), 2) == 0
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(ok), 6) == 0          # 96 x 128 -> 3 x 4
    assert L.mpc_iwe_pyramid_supported(None, 3) == _lib.E_NULL
    for levels in (-1, 0, 1, 7):
        assert L.mpc_iwe_pyramid_supported(ctypes.byref(ok), levels) == _lib.E_UNSUPPORTED, levels
        assert b'levels' in L.mpc_last_error_string()
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(flags=_lib.F_OBJ_VARIANCE)), 3) == _lib.E_UNSUPPORTED
    assert b'variance' in L.mpc_last_error_string()
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(T=2)), 3) == _lib.E_UNSUPPORTED
    assert b'num_tref' in L.mpc_last_error_string()
    # divisibility: 100 is not a multiple of 8; 98 not of 4; a coarsest level below 3x3
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(H=100, hq=25)), 4) == _lib.E_SHAPE
    assert b'divisible' in L.mpc_last_error_string()
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(W=98, wq=25)), 3) == _lib.E_SHAPE
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(H=8, W=8, hq=2, wq=2)), 3) == _lib.E_SHAPE
    assert L.mpc_iwe_pyramid_supported(ctypes.byref(_shape(H=12, W=12, hq=3, wq=3)), 3) == 0
    # the other two entry points refuse the same, before any launch
    assert L.mpc_iwe_pyramid_workspace_bytes(ctypes.byref(ok), 7, 1) == _lib.E_UNSUPPORTED
    assert L.mpc_iwe_pyramid_fwd(ctypes.byref(ok), 7, None, None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.mpc_iwe_pyramid_fwd(ctypes.byref(ok), 3, None, None, None, None, None, None, None) == _lib.E_NULL


def test_the_workspace_is_monotone_in_the_levels():
    from motionpriorcmax_amd import _lib, ops
    L = _lib.lib()
    s = _shape()
    for want_grad in (0, 1):
        sizes = [L.mpc_iwe_pyramid_workspace_bytes(ctypes.byref(s), lv, want_grad) for lv in range(2, 7)]
        # (without a gradient the workspace holds the band sums alone, rounded up to 256 bytes: it may stay level; with one every
        # level adds its adjoint image)
        assert sizes[0] > 0 and all((b > a) if want_grad else (b >= a) for a, b in zip(sizes, sizes[1:])), sizes
    n0, n1 = (L.mpc_iwe_pyramid_workspace_bytes(ctypes.byref(s), 3, g) for g in (0, 1))
    assert n1 > n0
    # the adjoint images come first, at the offsets the binding works out (include/mpcmax.h: the layout is part of the ABI)
    offs = ops.iwe_pyramid_level_offsets(s, 3)
    assert offs == [(0, (2, 48, 64)), (2 * 48 * 64, (2, 24, 32))]
    assert n1 - n0 >= 4 * (offs[-1][0] + 2 * 24 * 32)
