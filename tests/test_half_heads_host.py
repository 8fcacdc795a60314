"""The host side of the 16-bit network tensors of the head kernels (include/mpcmax.h: MPC_DT_*, the nine `_dt` entry points; no GPU):
the header declares them, the binding and the built library carry them, the version is unchanged; the bf16 rounding that the
kernels spell out (csrc/dt_device.h: mpc_bf16_bits) restated in NumPy equals torch.Tensor.to(torch.bfloat16) bit for bit; and the
CPU mirrors keep the dtype of their input."""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import ROOT

DT_ENTRY_POINTS = ('mpc_grid_traj_fwd_dt', 'mpc_grid_traj_bwd_dt', 'mpc_pe_tile_rows_dt', 'mpc_pe_tile_rows_bwd_dt', 'mpc_cvx_traj_fwd_dt',
                   'mpc_cvx_flow_fwd_dt', 'mpc_cvx_traj_bwd_dt', 'mpc_pec_head_rows_dt', 'mpc_pec_head_rows_bwd_dt')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)


def test_header_binding_and_library_carry_the_dt_entry_points():
    from motionpriorcmax_amd import _lib
    src = _header()
    for name, code in (('MPC_DT_F32', 0), ('MPC_DT_F16', 1), ('MPC_DT_BF16', 2)):
        assert re.search(r'#define %s %d\b' % (name, code), src), name
    assert (_lib.DT_F32, _lib.DT_F16, _lib.DT_BF16) == (0, 1, 2)
    assert re.search(r'#define MPC_VERSION 107\b', src) and _lib.lib().mpc_version() == 107
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in DT_ENTRY_POINTS:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, f'{name} is not declared'
        params = m.group(1)
        assert 'void *' in params and re.search(r'int32_t dtype\b', params), f'{name}: {params}'
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        # the fp32 call of the same name: one parameter fewer (the dtype code)
        base = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name[:-3], src)
        assert base and params.count(',') == base.group(1).count(',') + 1, name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-3]][1]) + 1


def _bf16_bits(x):
    """csrc/dt_device.h: mpc_bf16_bits, on an array of fp32 values -> uint16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def test_bf16_rounding_formula_equals_torch_bit_for_bit():
    rng = np.random.default_rng(7)
    bits = [
        np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000], dtype=np.uint32),    # ties to even, both ways
        np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000], dtype=np.uint32),                                                        # the largest finite value: rounds to inf
        np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000], dtype=np.uint32),   # +-0, subnormals
        np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF, 0xFFFFFFFF], dtype=np.uint32),   # +-inf, NaNs
        np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32),                                                                    # a sweep over every exponent
        (np.arange(0, 1 << 16, dtype=np.uint64) << 16 | 0x8000).astype(np.uint32),                                                          # every tie
        rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
    ]
    u = np.concatenate(bits)
    # torch's conversion is c10::BFloat16's round_to_nearest_even -- on the GPU always, on the CPU for a strided tensor; the CPU's
    # vector loop over a CONTIGUOUS tensor differs from it in the payload of a NaN alone (all ones), so the tensor is a strided view
    x = torch.from_numpy(np.stack((u, u), axis=1).view(np.float32))[:, 0]
    assert not x.is_contiguous()
    want = x.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)
    got = _bf16_bits(u.view(np.float32))
    nan = np.isnan(u.view(np.float32))
    assert int(nan.sum()) > 1000 and np.array_equal(got, want)
    assert bool((got[nan] == 0x7FC0).all())
    # the contiguous route: the same bits off the NaNs, and NaNs where NaNs went in
    cont = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16)
    assert np.array_equal(cont.view(torch.int16).numpy().view(np.uint16)[~nan], got[~nan]) and bool(torch.isnan(cont)[torch.from_numpy(nan)].all())


def test_cpu_mirrors_keep_the_dtype_of_their_input():
    from motionpriorcmax_amd import utils
    g = torch.Generator().manual_seed(0)
    grid = torch.randn(1, 1, 4, 16, 24, generator=g)
    times = torch.tensor([0.25, 0.75])
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        traj, pos = utils.trajectories_from_grid(grid.to(dt), times.to(dt), 2, 'polynomial', 4)
        assert traj.dtype == dt and tuple(traj.shape) == (1, 2, 24, 2) and pos.dtype == torch.int64
    params = torch.randn(1, 4, 2, 3, generator=g)
    mask = torch.randn(1, 576, 2, 3, generator=g)
    for dt in (torch.bfloat16, torch.float32):
        traj, _ = utils.trajectories_from_bezier(params.to(dt), [0.25, 0.75], 4, (16, 24), up_mask=mask.to(dt))
        assert traj.dtype == dt and tuple(traj.shape) == (1, 2, 24, 2)
        traj, _ = utils.trajectories_from_bezier(params.to(dt), [0.25, 0.75], 8, (16, 24))
        assert traj.dtype == dt and tuple(traj.shape) == (1, 2, 6, 2)
