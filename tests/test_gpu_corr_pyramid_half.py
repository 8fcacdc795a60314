"""The correlation pyramid from fp16 / bf16 feature maps (csrc/corr_pyramid.hip with mpc_f16 / mpc_bf16, through
utils.corr_pyramid_fused): level 0 on v_mfma_f32_32x32x16_f16 / _bf16, everything else the fp32 kernels with the 16-bit element
converted at the load.  Inputs and references: tests/corr_pyramid_cases.py (PK), tests/corr_pyramid_multi_cases.py (PM),
tests/corr_pyramid_half_cases.py (HK).

  1. every case of PK: the levels are fp32 and equal PK.expected(name).levels bit for bit (the inputs are exact in both 16-bit types and
     every partial sum of every order is exact in fp32, so the other summation order of level 0 has to give the same bits);
  2. levels >= 1 and both gradients equal the fp32 node run on fmap.float(), the gradients rounded with .to(dtype), bit for bit: every
     case of PK, PK's missing-cotangent sets, the list form on every case of PM (which also equals its R single-reference nodes,
     level 0 included);
  3. level 0 on randn data rounded to the dtype against float64 under gamma(D) * A with u = 2^-23, the levels above with u = 2^-24;
  4. maps that start 1, 2 and 4 elements into their storage give the bits of the aligned run;
  5. fp16 subnormal inputs are multiplied as the values they are;
  6. mixed dtypes run the fp32 node on upcast inputs, every gradient in its input's dtype;
  7. no host synchronisation, two runs bitwise equal, capture and replay, an empty batch."""
import pytest
import torch

import corr_pyramid_cases as PK
import corr_pyramid_half_cases as HK
import corr_pyramid_multi_cases as PM

pytestmark = pytest.mark.gpu

DT = sorted(HK.DTYPES)


def _dev():
    return torch.device('cuda', 0)


def _bits(a, b):
    """Same dtype, shape and bits."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _put(t, dtype=torch.float32, shift=0):
    """The CPU fp32 tensor on the device in `dtype` (exact: asserted); shift: as a contiguous view that starts `shift` elements into
    a larger storage."""
    h = HK.as_dtype(t, dtype)
    if not shift:
        return h.to(_dev()).contiguous()
    buf = torch.zeros(h.numel() + 8, dtype=dtype, device=_dev())
    v = buf[shift:shift + h.numel()].view(h.shape)
    v.copy_(h)
    assert v.is_contiguous() and v.data_ptr() % 16 == (shift * h.element_size()) % 16
    return v


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items() if k.startswith('k_corr_pyr')}


def _pyramid(f1, f2, nl, cot, missing=(), node='CorrPyramidFn'):
    """Forward and backward through utils.corr_pyramid_fused (tensor form, or list form with f1 / f2 lists) ->
    (levels, gradients of f1 then f2 in order, launches)."""
    from motionpriorcmax_amd import ops, utils
    many = isinstance(f1, (list, tuple))
    ins = [t.detach().requires_grad_(True) for t in (list(f1) + list(f2) if many else [f1, f2])]
    n = len(ins) // 2
    with ops.KernelTimer() as kt:
        levels, _ = utils.corr_pyramid_fused(ins[:n], ins[n:], nl) if many else utils.corr_pyramid_fused(ins[0], ins[1], nl)
        assert all(type(lv.grad_fn).__name__.startswith(node) for lv in levels), [type(lv.grad_fn).__name__ for lv in levels]
        keep = [l for l in range(len(levels)) if l not in missing]
        grads = torch.autograd.grad([levels[l] for l in keep], ins, [cot[l] for l in keep])
    return [lv.detach() for lv in levels], list(grads), _launches(kt)


_RUN = {}


def _case_run(name, key, missing=()):
    """PK.case(name) in dtype `key` ('fp32': the fp32 node on the upcast maps -- the same numbers), computed once."""
    k = (name, key, tuple(missing))
    if k not in _RUN:
        cs = PK.case(name)
        dtype = HK.DTYPES.get(key, torch.float32)
        _RUN[k] = _pyramid(_put(cs.f1, dtype), _put(cs.f2, dtype), cs.nl, [_put(c) for c in cs.cot], missing)
    return _RUN[k]


def _assert_same_as_upcast(label, half, full, dtype, level0=False):
    """levels >= 1 (and level 0 where `level0`) and every gradient of the 16-bit run against the fp32 run: bit for bit."""
    (lv, gr, _), (lw, gw, _) = half, full
    assert len(lv) == len(lw) and len(gr) == len(gw)
    for l in range(0 if level0 else 1, len(lv)):
        assert lv[l].dtype == torch.float32 and _bits(lv[l], lw[l]), f'{label}: level {l}'
    for i, (a, b) in enumerate(zip(gr, gw)):
        assert a.dtype == dtype and b.dtype == torch.float32 and a.is_contiguous(), f'{label}: gradient {i} is {a.dtype}'
        assert _bits(a, b.to(dtype)), f'{label}: gradient {i}'


# ---- 1. the exact bank, forward
@pytest.mark.parametrize('name', PK.CASES)
@pytest.mark.parametrize('key', DT)
def test_levels_of_the_exact_bank_bit_for_bit(key, name):
    cs = PK.case(name)
    levels, _, launches = _case_run(name, key)
    want = {'k_corr_pyr_gemm16': 1, 'k_corr_pyr_gather': 1, 'k_corr_pyr_gemm': 2 + int(cs.L > 1)}
    if cs.L > 1:
        want['k_corr_pyr_pool'] = 2 * (cs.L - 1)
    if cs.S > 1:
        want['k_corr_pyr_reduce'] = 1
    assert launches == want, launches
    for l, lv in enumerate(levels):
        assert lv.dtype == torch.float32 and lv.is_contiguous() and tuple(lv.shape) == (len(cs.tix[l]), cs.B * cs.hw, 1, cs.h >> l, cs.w >> l)
    PK.compare_all(f'{name} {key}', name, levels=levels)


# ---- 2. the same bits as the upcast route where the arithmetic is the same
@pytest.mark.parametrize('name,missing', [(n, ()) for n in PK.CASES] + [(n, PK.MISSING[n][0]) for n in sorted(PK.MISSING)])
@pytest.mark.parametrize('key', DT)
def test_levels_above_0_and_gradients_are_the_fp32_node_on_the_upcast_maps(key, name, missing):
    half, full = _case_run(name, key, missing), _case_run(name, 'fp32', missing)
    # (level 0 too: on these inputs every order of the sum gives the same bits)
    _assert_same_as_upcast(f'{name} {key} without {list(missing)}', half, full, HK.DTYPES[key], level0=True)
    assert all(float(g.float().abs().max()) > 0 for g in half[1])
    # the fp32 run is itself the reference's (the gradients under PK's bound where sqrt(D) is no power of two)
    PK.compare_all(f'{name} fp32', name, missing, levels=None if missing else full[0], g1=full[1][0], g2=full[1][1])


def _multi_inputs(cs, dtypes):
    return [_put(t, d) for t, d in zip(cs.f1, dtypes)], [_put(t, d) for t, d in zip(cs.f2, dtypes)]


@pytest.mark.parametrize('name,missing', [(n, ()) for n in PM.CASES] + [(n, PM.MISSING[n]) for n in sorted(PM.MISSING)])
@pytest.mark.parametrize('key', DT)
def test_the_list_form_is_the_fp32_list_node_and_its_single_reference_nodes(key, name, missing):
    cs, dtype = PM.case(name), HK.DTYPES[key]
    cot = [_put(c) for c in cs.cot]
    half = _pyramid(*_multi_inputs(cs, [dtype] * cs.R), cs.nls, cot, missing, node='CorrPyramidMultiFn')
    full = _pyramid(*_multi_inputs(cs, [torch.float32] * cs.R), cs.nls, cot, missing, node='CorrPyramidMultiFn')
    assert half[2].get('k_corr_pyr_gemm16') == 1 and 'k_corr_pyr_gemm16' not in full[2], (half[2], full[2])
    _assert_same_as_upcast(f'{name} {key} list form without {list(missing)}', half, full, dtype, level0=True)
    if not missing:
        PM.compare_all(f'{name} {key} list form', name, levels=half[0])
    # the R single-reference 16-bit nodes: level 0 included, bit for bit
    for r in range(cs.R):
        rc = PM.reference_case(cs, r)
        miss = tuple(l for l in missing if l < rc.L)
        if len(miss) == rc.L:
            continue
        one = _pyramid(_put(rc.f1, dtype), _put(rc.f2, dtype), rc.nl, [_put(c) for c in rc.cot], miss)
        for l in range(rc.L):
            s0, n = PM.slots(cs, r, l)
            assert _bits(half[0][l][s0:s0 + n], one[0][l]), f'{name} {key}: level {l} of reference {r}'
        assert _bits(half[1][r], one[1][0]) and _bits(half[1][cs.R + r], one[1][1]), f'{name} {key}: gradients of reference {r}'


# ---- 3. level 0 on data that is not exact
_RANDN = {}


def _randn_reference(shape):
    """randn rounded to the 16-bit type -> float64 levels through utils.corr_pyramid on the upcast values, and the same on absolute
    values (A): computed once per (shape, dtype)."""
    from motionpriorcmax_amd import utils
    out = {}
    B, D, h, w, nl = shape
    g = torch.Generator().manual_seed(31 + D)
    a, b = torch.randn(B, D, h, w, generator=g), torch.randn(len(nl), B, D, h, w, generator=g)
    for key, dtype in HK.DTYPES.items():
        f1, f2 = a.to(dtype), b.to(dtype)
        ref, _ = utils.corr_pyramid(f1.double(), f2.double(), nl)
        mag, _ = utils.corr_pyramid(f1.double().abs(), f2.double().abs(), nl)
        out[key] = (f1, f2, ref, mag)
    return out


@pytest.mark.parametrize('shape', HK.RANDN_SHAPES, ids=lambda s: f'D{s[1]}')
@pytest.mark.parametrize('key', DT)
def test_level_0_on_inexact_data_under_the_derived_bound(key, shape):
    from motionpriorcmax_amd import utils
    sk = (shape[:4], tuple(shape[4]))
    if sk not in _RANDN:
        _RANDN[sk] = _randn_reference(shape)
    f1, f2, ref, mag = _RANDN[sk][key]
    B, D, h, w, nl = shape
    levels, _ = utils.corr_pyramid_fused(f1.to(_dev()), f2.to(_dev()), nl)
    worst = []
    for l, lv in enumerate(levels):
        assert lv.dtype == torch.float32
        err = (lv.cpu().double() - ref[l]).abs()
        bound = HK.gamma(D, HK.U_LEVEL0 if l == 0 else HK.U_ABOVE) * mag[l]
        worst.append(float((err / bound).max()))
        print(f'{key} D {D} level {l}: max |err| {float(err.max()):.4g}, largest err / bound {worst[-1]:.4g}', flush=True)
    for l, lv in enumerate(levels):
        err = (lv.cpu().double() - ref[l]).abs()
        assert bool((err <= HK.gamma(D, HK.U_LEVEL0 if l == 0 else HK.U_ABOVE) * mag[l]).all()), (key, D, l, worst)
    # the levels above 0 are the fp32 node's on the upcast maps
    up, _ = utils.corr_pyramid_fused(f1.float().to(_dev()), f2.float().to(_dev()), nl)
    assert all(_bits(a, b) for a, b in zip(levels[1:], up[1:]))


# ---- 4. addresses
@pytest.mark.parametrize('shift', HK.ADDRESS_SHIFTS)
@pytest.mark.parametrize('name', HK.ADDRESS_CASES)
@pytest.mark.parametrize('key', DT)
def test_maps_that_start_off_a_16_byte_boundary_give_the_same_bits(key, name, shift):
    cs, dtype = PK.case(name), HK.DTYPES[key]
    f1, f2 = _put(cs.f1, dtype, shift), _put(cs.f2, dtype, shift)
    assert f1.data_ptr() % 16 == 2 * shift and f2.data_ptr() % 16 == 2 * shift
    got = _pyramid(f1, f2, cs.nl, [_put(c) for c in cs.cot])
    want = _case_run(name, key)
    assert all(_bits(a, b) for a, b in zip(got[0], want[0])), f'{name} {key} + {shift}: levels'
    assert all(_bits(a, b) for a, b in zip(got[1], want[1])), f'{name} {key} + {shift}: gradients'


# ---- 5. fp16 subnormals
def test_fp16_subnormal_inputs_are_multiplied_as_the_values_they_are():
    from motionpriorcmax_amd import utils
    cs = PK.case('interior')
    f1 = cs.f1 * 2.0 ** -24                                       # every element an fp16 subnormal or zero
    assert bool((f1.abs() < 2.0 ** -14).all())
    levels, _ = utils.corr_pyramid_fused(_put(f1, torch.float16), _put(cs.f2, torch.float16), cs.nl)
    e = PK.expected('interior')
    for l, lv in enumerate(levels):
        want = e.levels[l] * 2.0 ** -24
        assert torch.equal(want.double(), e.levels[l].double() * 2.0 ** -24) and float(want.abs().max()) > 0
        PK.compare('interior * 2^-24 fp16', f'level_{l}', lv, want, B=cs.B)


# ---- 6. mixed dtypes
def test_fp32_fmap1_with_bf16_fmap2_is_the_fp32_node_on_upcast_inputs():
    cs = PK.case('mixed')
    cot = [_put(c) for c in cs.cot]
    got = _pyramid(_put(cs.f1), _put(cs.f2, torch.bfloat16), cs.nl, cot)
    want = _case_run('mixed', 'fp32')
    assert 'k_corr_pyr_gemm16' not in got[2] and got[2] == want[2], got[2]
    assert all(_bits(a, b) for a, b in zip(got[0], want[0]))
    assert got[1][0].dtype == torch.float32 and _bits(got[1][0], want[1][0])
    assert got[1][1].dtype == torch.bfloat16 and _bits(got[1][1], want[1][1].to(torch.bfloat16))


def test_a_bf16_reference_beside_an_fp32_reference_is_the_fp32_list_node():
    cs = PM.case('stops_at_0')
    cot = [_put(c) for c in cs.cot]
    dts = [torch.bfloat16, torch.float32]
    got = _pyramid(*_multi_inputs(cs, dts), cs.nls, cot, node='CorrPyramidMultiFn')
    want = _pyramid(*_multi_inputs(cs, [torch.float32] * 2), cs.nls, cot, node='CorrPyramidMultiFn')
    assert 'k_corr_pyr_gemm16' not in got[2] and got[2] == want[2], got[2]
    assert all(_bits(a, b) for a, b in zip(got[0], want[0]))
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        assert a.dtype == dts[i % 2] and _bits(a, b.to(dts[i % 2])), i


# ---- 7. housekeeping
def _step(f1, f2, nl, cot):
    from motionpriorcmax_amd import utils
    a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
    levels, _ = utils.corr_pyramid_fused(a, b, nl)
    return tuple(lv.detach() for lv in levels) + tuple(torch.autograd.grad(levels, [a, b], cot))


def _step_args(key, name='interior'):
    cs, dtype = PK.case(name), HK.DTYPES[key]
    return _put(cs.f1, dtype), _put(cs.f2, dtype), cs.nl, [_put(c) for c in cs.cot]


@pytest.mark.parametrize('key', DT)
def test_no_host_synchronisation(key):
    args = _step_args(key)
    _step(*args)                                                 # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _step(*args)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out[-2].dtype == args[0].dtype and out[-1].shape == args[1].shape


@pytest.mark.parametrize('name', PK.REPEAT_CASES)
@pytest.mark.parametrize('key', DT)
def test_two_runs_are_bitwise_equal(key, name):
    args = _step_args(key, name)
    a, b = _step(*args), _step(*args)
    assert all(_bits(x, y) for x, y in zip(a, b)) and all(float(x.float().abs().max()) > 0 for x in a)


@pytest.mark.parametrize('key', DT)
def test_capture_replays_bitwise_equal_to_eager(key):
    """Forward + backward captured into a torch.cuda.graph on one stream and replayed (the pattern of test_gpu_corr_pyramid.py)."""
    args = _step_args(key)
    eager = [t.clone() for t in _step(*args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture
        for _ in range(2):
            _step(*args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(*args)
    graph.replay()
    torch.cuda.synchronize()
    assert len(static) == len(eager) and all(_bits(a, b) for a, b in zip(static, eager))


@pytest.mark.parametrize('key', DT)
def test_an_empty_batch_launches_nothing(key):
    from motionpriorcmax_amd import ops, utils
    dev, dtype = _dev(), HK.DTYPES[key]
    f1 = torch.zeros(0, 16, 6, 8, device=dev, dtype=dtype, requires_grad=True)
    f2 = torch.zeros(2, 0, 16, 6, 8, device=dev, dtype=dtype, requires_grad=True)
    with ops.KernelTimer() as kt:
        levels, tix = utils.corr_pyramid_fused(f1, f2, [2, 1])
        g1, g2 = torch.autograd.grad([lv.sum() for lv in levels], [f1, f2])
    assert kt.summary() == {}
    assert tix == [[0, 1], [0]] and [tuple(lv.shape) for lv in levels] == [(2, 0, 1, 6, 8), (1, 0, 1, 3, 4)]
    assert all(lv.dtype == torch.float32 and type(lv.grad_fn).__name__.startswith('CorrPyramidFn') for lv in levels)
    assert g1.shape == f1.shape and g2.shape == f2.shape and g1.dtype == dtype and g2.dtype == dtype
