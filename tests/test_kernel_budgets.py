"""Register, scratch and LDS budgets of the kernels whose occupancy the step time rests on, read from the metadata notes of the code
objects inside libmpcmax.so (llvm-readelf --notes, as tools/kernel_resources.py does; never the instruction stream).  No GPU needed.

A change that looks free at the source level -- a scheduling fence such as the priority builtin behind MPC_PRIO, one more live value --
can move the register allocation: k_lut_accum<false> once drifted to 81 VGPRs, one over the 80 of six wavefronts per SIMD, and lost a
workgroup per CU unnoticed.  Three assertions per kernel:
  * registers: vgpr_count (+ agpr_count: one file on this chip) is at most the largest count that still allows the wavefronts per SIMD
    the kernel's __launch_bounds__ asks for -- 512 registers per lane and SIMD, handed out in blocks of 8: 64 / 72 / 80 / 96 / 128 for
    8 / 7 / 6 / 5 / 4 wavefronts;
  * spills: vgpr_spill_count and private_segment_fixed_size (scratch bytes per lane) are not above the RECORDED figures below;
  * static LDS: group_segment_fixed_size equals the recorded figure.
The recorded figures are those of commit d2a17ae (the parent of the commit that added this file), taken with tools/kernel_resources.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from motionpriorcmax_amd import build

VGPR_LIMIT = {8: 64, 7: 72, 6: 80, 5: 96, 4: 128}


def _llvm_bin():
    hipcc = os.path.realpath(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
    for d in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'lib', 'llvm', 'bin'), '/opt/rocm/lib/llvm/bin', '/opt/rocm/llvm/bin'):
        if os.path.exists(os.path.join(d, 'llvm-readelf')):
            return d
    raise RuntimeError('llvm-readelf of the ROCm toolchain not found')


# wavefronts per SIMD of every instantiation: the second argument of the kernel's __launch_bounds__ with the defaults of csrc/tuning.h
# (256-thread workgroups: one wavefront per SIMD, so workgroups per CU = wavefronts per SIMD)
def _waves(name):
    m = re.match(r'(\w+)(?:<(.*)>)?$', name)
    kern, args = m.group(1), [a.strip() for a in (m.group(2) or '').split(',')]
    if kern == 'k_knn_strip':           # <L1, NEXT, IWD>: (NEXT || L1) ? KS_OCC_WIDE = 5 : 6
        return 5 if 'true' in args[0:2] else 6
    if kern == 'k_knn_tail':            # KS_MORE_OCC = 4
        return 4
    if kern == 'k_knn_bwd_tile':        # <L1, NEXT, IWD>: NEXT ? KNN_BW_OCC_NEXT = 6 : (IWD ? KNN_BW_OCC_IWD = 7 : KNN_BW_OCC = 7)
        return 6 if args[1] == 'true' else 7
    if kern == 'k_lut_accum':           # <false>: EV_LUT_MINWAVES = 6 (three 512-thread workgroups per CU)
        return 6
    if kern == 'k_contrast_smooth_march':   # __launch_bounds__(64) names no count: held to the 8 wavefronts per SIMD it runs at
        return 8
    raise KeyError(name)


# name: (vgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size) of the parent commit
RECORDED = {
    'k_knn_strip<false, false, false>': (0, 0, 432),
    'k_knn_strip<false, false, true>': (1, 8, 432),
    'k_knn_strip<false, true, false>': (1, 8, 432),
    'k_knn_strip<false, true, true>': (11, 48, 432),
    'k_knn_strip<true, false, false>': (0, 0, 432),
    'k_knn_strip<true, false, true>': (0, 0, 432),
    'k_knn_strip<true, true, false>': (9, 40, 432),
    'k_knn_strip<true, true, true>': (23, 96, 432),
    'k_knn_tail<false, false, false>': (14, 60, 880),
    'k_knn_tail<false, false, true>': (20, 84, 880),
    'k_knn_tail<false, true, false>': (32, 128, 880),
    'k_knn_tail<false, true, true>': (48, 168, 880),
    'k_knn_tail<true, false, false>': (16, 60, 880),
    'k_knn_tail<true, false, true>': (21, 84, 880),
    'k_knn_tail<true, true, false>': (36, 124, 880),
    'k_knn_tail<true, true, true>': (56, 168, 880),
    'k_knn_bwd_tile<false, false, false>': (2, 12, 272),
    'k_knn_bwd_tile<false, false, true>': (2, 12, 272),
    'k_knn_bwd_tile<false, true, false>': (10, 44, 272),
    'k_knn_bwd_tile<false, true, true>': (17, 72, 272),
    'k_knn_bwd_tile<true, false, false>': (2, 12, 272),
    'k_knn_bwd_tile<true, false, true>': (2, 12, 272),
    'k_knn_bwd_tile<true, true, false>': (10, 44, 272),
    'k_knn_bwd_tile<true, true, true>': (17, 72, 272),
    'k_lut_accum<false>': (0, 0, 0),
    'k_contrast_smooth_march<false, 16, 16>': (0, 0, 0),
    'k_contrast_smooth_march<false, 16, 8>': (0, 0, 0),
    'k_contrast_smooth_march<false, 32, 16>': (0, 0, 0),
    'k_contrast_smooth_march<false, 32, 8>': (0, 0, 0),
    'k_contrast_smooth_march<true, 16, 16>': (0, 0, 0),
    'k_contrast_smooth_march<true, 16, 8>': (0, 0, 0),
    'k_contrast_smooth_march<true, 32, 16>': (0, 0, 0),
    'k_contrast_smooth_march<true, 32, 8>': (0, 0, 0),
}
FAMILIES = ('k_knn_strip<', 'k_knn_tail<', 'k_knn_bwd_tile<', 'k_lut_accum<false>', 'k_contrast_smooth_march<')


@pytest.fixture(scope='module')
def kernels():
    """{demangled kernel name without its parameter list: {field: int}} of every kernel of the library."""
    lib = build.build_library()          # (a no-op when the library is up to date)
    llvm = _llvm_bin()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        # every source file is one bundle inside the fat binary; llvm-objdump extracts them next to its input: work on a copy
        copy = shutil.copy(lib, os.path.join(td, 'lib.so'))
        subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', copy], cwd=td, capture_output=True, text=True, check=True)
        objs = [f for f in os.listdir(td) if 'gfx950' in f]
        assert objs, 'no gfx950 code object in ' + lib
        for f in objs:
            notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', os.path.join(td, f)], capture_output=True, text=True, check=True).stdout
            blocks = notes.split('- .agpr_count:')[1:]
            mangled = [re.search(r'\.name:\s+(\S+)', b).group(1) for b in blocks]
            filt = os.path.join(llvm, 'llvm-cxxfilt') if os.path.exists(os.path.join(llvm, 'llvm-cxxfilt')) else shutil.which('c++filt')
            assert filt, 'no demangler (llvm-cxxfilt, c++filt)'
            names = subprocess.run([filt] + mangled, capture_output=True, text=True, check=True).stdout.split('\n')
            for blk, dem in zip(blocks, names):
                name = dem.split('(')[0].replace('void ', '').strip()
                rec = {'agpr_count': int(blk.split()[0])}
                for k in ('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size'):
                    rec[k] = int(re.search(r'\.' + k + r':\s+(\d+)', blk).group(1))
                out[name] = rec
    return out


def test_every_instantiation_is_recorded(kernels):
    """The table above names exactly the instantiations of the five kernel families the library holds: a new one gets its line."""
    have = sorted(n for n in kernels if n.startswith(FAMILIES))
    assert have == sorted(RECORDED)


@pytest.mark.parametrize('name', sorted(RECORDED))
def test_kernel_budget(kernels, name):
    k = kernels[name]
    spill, scratch, lds = RECORDED[name]
    waves = _waves(name)
    print(name, k, 'wavefronts per SIMD asked for:', waves)
    assert k['vgpr_count'] + k['agpr_count'] <= VGPR_LIMIT[waves], f'{name}: registers beyond the {VGPR_LIMIT[waves]} of {waves} wavefronts per SIMD'
    assert k['vgpr_spill_count'] <= spill
    assert k['private_segment_fixed_size'] <= scratch
    assert k['group_segment_fixed_size'] == lds
