"""The host side of the correlation pyramid from fp16 / bf16 feature maps (include/mpcmax.h: the four mpc_corr_pyramid_*_dt entry
points; no GPU): the header declares them, the binding and the built library carry them, the version is unchanged; an unknown dtype
code is refused with its error string before anything else happens, the descriptor checks are those of the fp32 calls; the cases of
tests/corr_pyramid_cases.py are exact in both 16-bit types; and those cases with the address variants reach every branch of the
level-0 loader (tests/corr_pyramid_half_cases.py: level0_paths)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import corr_pyramid_cases as PK
import corr_pyramid_half_cases as HK
import corr_pyramid_multi_cases as PM


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)


def test_header_binding_and_library_carry_the_dt_entry_points():
    from motionpriorcmax_amd import _lib
    src = _header()
    assert re.search(r'#define MPC_VERSION 107\b', src) and _lib.lib().mpc_version() == 107
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in HK.DT_ENTRY_POINTS:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, f'{name} is not declared'
        params = m.group(1)
        assert re.search(r'\bint(32_t)? dtype\b', params), f'{name}: {params}'
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        # the fp32 call of the same name: one parameter fewer (the dtype code), the maps typed float there and void here
        base = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name[:-3], src)
        assert base and params.count(',') == base.group(1).count(',') + 1, name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-3]][1]) + 1
        assert 'float' not in params and ('multi' in name or 'const void *fmap1' in params), f'{name}: {params}'


def _desc(**kw):
    from motionpriorcmax_amd import ops
    args = dict(B=1, h=8, w=8, nl=[2, 1])
    args.update(kw)
    return ops.corr_pyramid_desc(args['B'], args['h'], args['w'], args['nl'])[0]


def _calls(L, desc, D, dtype):
    from motionpriorcmax_amd import ops
    refs = ops.corr_pyramid_refs([2])
    d = ctypes.byref(desc)
    return {'mpc_corr_pyramid_fwd_dt': lambda: L.mpc_corr_pyramid_fwd_dt(d, D, None, None, dtype, None, None),
            'mpc_corr_pyramid_bwd_dt': lambda: L.mpc_corr_pyramid_bwd_dt(d, D, None, None, None, None, dtype, None, None),
            'mpc_corr_pyramid_multi_fwd_dt': lambda: L.mpc_corr_pyramid_multi_fwd_dt(d, D, ctypes.byref(refs), dtype, None, None),
            'mpc_corr_pyramid_multi_bwd_dt': lambda: L.mpc_corr_pyramid_multi_bwd_dt(d, D, ctypes.byref(refs), dtype, None, None)}


@pytest.mark.parametrize('code', [3, -1, 7])
def test_an_unknown_dtype_code_is_refused_with_its_error_string(code):
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    for name, call in _calls(L, _desc(), 64, code).items():
        assert call() == _lib.E_UNSUPPORTED, name
        msg = L.mpc_last_error_string()
        assert name.encode() in msg and b'unknown dtype code %d' % code in msg and b'MPC_DT_BF16' in msg, msg


@pytest.mark.parametrize('code', [0, 1, 2])
def test_the_known_codes_run_the_checks_of_the_fp32_calls(code):
    from motionpriorcmax_amd import _lib
    L = _lib.lib()
    for name, call in _calls(L, _desc(), 6, code).items():                 # D is no multiple of 4
        assert call() == _lib.E_UNSUPPORTED and b'multiple of 4' in L.mpc_last_error_string(), name
    for name, call in _calls(L, _desc(B=0), 64, code).items():             # B = 0: nothing to do, nothing is read
        assert call() == 0, name
    for name, call in _calls(L, _desc(), 64, code).items():
        if name.endswith('fwd_dt'):                                        # null maps (a backward without a wanted gradient returns 0)
            assert call() == _lib.E_NULL, name
    # the queries do not take a dtype: one workspace whatever the element type
    assert not any(n.startswith('mpc_corr_pyramid') and 'workspace' in n and n.endswith('_dt') for n in _lib.SIGNATURES)


def test_the_case_banks_are_exact_in_both_16_bit_types():
    for dtype in HK.DTYPES.values():
        for name in PK.CASES:
            cs = PK.case(name)
            HK.as_dtype(cs.f1, dtype), HK.as_dtype(cs.f2, dtype)
        for name in PM.CASES:
            cs = PM.case(name)
            for t in cs.f1 + cs.f2:
                HK.as_dtype(t, dtype)
    # the subnormal case: every element of 2^-24 * fmap1 is an fp16 subnormal or zero, and exact
    f1 = PK.case('interior').f1 * 2.0 ** -24
    h = f1.to(torch.float16)
    assert torch.equal(h.float(), f1) and bool((h.float().abs() < 2.0 ** -14).all()) and bool((h != 0).any())


def test_the_cases_reach_every_branch_of_the_level_0_loader():
    reached = {}
    for name in PK.CASES:
        for b in HK.level0_paths(name):
            reached.setdefault(b, []).append(name)
    for name in HK.ADDRESS_CASES:
        for s in HK.ADDRESS_SHIFTS:
            paths = HK.level0_paths(name, s)
            assert 'narrow' in paths and 'interior' not in paths and 'wide_ragged' not in paths, (name, s, paths)
            for b in paths:
                reached.setdefault(b, []).append(f'{name}+{s}')
    for b in HK.LOADER_BRANCHES:
        print(f'{b}: {reached.get(b, [])}')
    assert set(reached) == set(HK.LOADER_BRANCHES), set(HK.LOADER_BRANCHES) - set(reached)
    # each branch by a case of the aligned bank alone, too: the address variants add the narrow loads at 16-byte friendly shapes
    assert 'interior' in HK.level0_paths('interior') and HK.level0_paths('interior') == {'interior'}
    assert {'ragged_m', 'ragged_n', 'wide_ragged'} <= HK.level0_paths('mixed')
    assert {'k_remainder', 'half_step'} <= HK.level0_paths('d8') and {'k_remainder', 'half_step'} <= HK.level0_paths('d132')
    assert {'narrow', 'narrow_tail'} <= HK.level0_paths('six_levels')
    assert 'half_step' not in HK.level0_paths('d160') and 'k_remainder' not in HK.level0_paths('d512')


def test_routing_off_the_gpu_is_unchanged():
    """CPU tensors keep going to the plain-torch mirror, which keeps the dtype of its input."""
    from motionpriorcmax_amd import utils
    cs = PK.case('offset')
    for dtype in (torch.bfloat16, torch.float32):
        levels, tix = utils.corr_pyramid_fused(cs.f1.to(dtype), cs.f2.to(dtype), cs.nl)
        want, _ = utils.corr_pyramid(cs.f1.to(dtype), cs.f2.to(dtype), cs.nl)
        assert tix == cs.tix and all(a.dtype == dtype and torch.equal(a, b) for a, b in zip(levels, want))
