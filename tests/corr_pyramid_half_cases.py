"""What the 16-bit route of the correlation pyramid (csrc/corr_pyramid.hip with mpc_f16 / mpc_bf16 feature maps; the `_dt` entry points of
include/mpcmax.h) is tested with, shared by tests/test_corr_pyramid_half_host.py (CPU) and tests/test_gpu_corr_pyramid_half.py.

The inputs are those of tests/corr_pyramid_cases.py (PK) and tests/corr_pyramid_multi_cases.py (PM): integers in [-2, 2], exact in
fp16 and in bf16 (`as_dtype` asserts the round trip), for which PK's precondition makes every partial sum of every order exact in fp32
-- so level 0, which the 16-bit route sums on v_mfma_f32_32x32x16_f16 / _bf16 in another order than the fp32 kernel, has to equal
PK.expected(name).levels[0] bit for bit like every other level.

`level0_paths` restates the tile decode and the loader of k_corr_pyr_gemm16 and records which of its branches a case takes.  The
loader's branches, per operand tile and k block of 32 channels (A = fmap1 along m, B = fmap2 along n):

  interior     16-byte loads allowed (the map 16-byte aligned, h * w a multiple of 8), 128 valid m / n, 32 valid k: four loads, no
               predicate
  ragged_m     fewer than 128 valid m in an A tile: the chunks of 8 past the end are zeros
  ragged_n     the same along n in a B tile
  k_remainder  fewer than 32 valid k in the block: the rows beyond D are zeros
  half_step    ... of which D is no multiple of 16: a 16-deep MFMA step that is partly zeros (D = 8, 132)
  wide_ragged  a ragged tile or block whose valid chunks still load 16 bytes
  narrow       16-byte loads not allowed (odd h * w, or a view that starts 1, 2 or 4 elements into its storage): 8 element loads
  narrow_tail  ... of which a chunk that holds fewer than 8 valid m / n (h * w no multiple of 8)
"""
import torch

import corr_pyramid_cases as PK

DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
DT_CODE = {'fp16': 1, 'bf16': 2}                                   # MPC_DT_F16, MPC_DT_BF16
DT_ENTRY_POINTS = ('mpc_corr_pyramid_fwd_dt', 'mpc_corr_pyramid_bwd_dt', 'mpc_corr_pyramid_multi_fwd_dt', 'mpc_corr_pyramid_multi_bwd_dt')
BM, HK = 128, 32                                                   # CP_BM, CP_HK
LOADER_BRANCHES = ('interior', 'ragged_m', 'ragged_n', 'k_remainder', 'half_step', 'wide_ragged', 'narrow', 'narrow_tail')
ADDRESS_CASES = ('interior', 'offset')
ADDRESS_SHIFTS = (1, 2, 4)                                         # elements into the storage: 2, 4 and 8 bytes off a 16-byte boundary

# level 0 on data that is not exact: B, D, h, w, level counts
RANDN_SHAPES = ((2, 132, 9, 16, [1, 2]), (1, 256, 8, 20, [2]), (1, 512, 4, 36, [1]))
U_LEVEL0 = 2.0 ** -23                                              # an adder of unspecified rounding: one ulp per addition
U_ABOVE = 2.0 ** -24                                               # the fp32 kernel: half an ulp (tests/test_gpu_corr_pyramid.py)


def gamma(n, u):
    return (n + 8) * u / (1.0 - (n + 8) * u)


def as_dtype(t, dtype):
    """The fp32 integers of a case in `dtype`, the round trip asserted: the 16-bit tensor holds the same numbers."""
    h = t.to(dtype)
    assert torch.equal(h.float(), t), 'the case is not exact in ' + str(dtype)
    return h


def level0_paths(name, shift=0):
    """The loader branches k_corr_pyr_gemm16 takes for PK.case(name) with both maps starting `shift` elements off a 16-byte boundary:
    (slot, sample, tile m, tile n) as the kernel decodes them, every k block of both operands."""
    cs = PK.case(name)
    hw, D = cs.hw, cs.D
    vec = hw % 8 == 0 and (2 * shift) % 16 == 0
    tm = PK.cdiv(hw, BM)
    paths = set()
    for bid in range(len(cs.tix[0]) * cs.B * tm * tm):
        in_, im = bid % tm, (bid // tm) % tm
        for rem, ragged in ((hw - im * BM, 'ragged_m'), (hw - in_ * BM, 'ragged_n')):
            for kb in range(0, D, HK):
                if vec and rem >= BM and kb + HK <= D:
                    paths.add('interior')
                    continue
                if rem < BM:
                    paths.add(ragged)
                if D - kb < HK:
                    paths.add('k_remainder')
                    if D % 16:
                        paths.add('half_step')
                if vec:
                    paths.add('wide_ragged')
                else:
                    paths.add('narrow')
                    if min(rem, BM) % 8:
                        paths.add('narrow_tail')
    return paths
