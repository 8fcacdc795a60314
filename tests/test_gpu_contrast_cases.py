"""The contrast and smoothness kernels (csrc/contrast.hip) element by element against the float64 reference of
tests/contrast_cases.py, through the stage wrappers of ops.py: the marching contrast kernel (blur, adjoint image, the five scalars,
l1 and l2, both band heights, 8400 partial-sum slots of which 5600 are used), the LDS-tiled forward-only path, the variance
objective with its adjoint, the marching smoothness kernel (SMOOTH and grad_field, both band heights, C = 2 and 6, with and
without a gradient, 8202 partial sums), the 2x2 pooling pair at odd sizes with coefficient ratios 0, inf and NaN, and mpc_scale.

Every bound is the running error bound derived in tests/contrast_cases.py from the roundings counted in the kernels; the l1
adjoint image has the accountable allowance described there.  No element is excused; the figures are printed before they are
asserted (pytest -s).

The workspace is filled with 0xFF bytes (NaN as float and double) before every call.  From the code: mpc_contrast_fwd writes every
one of the n_cblocks partial-sum slots (the marching kernel clears those its tiling does not use, the LDS-tiled path zeroes the
array first) and, for the variance adjoint, the per-image means before it reads them; mpc_lut_smooth writes exactly the partial
sums mpc_finalize adds.  mpc_finalize after mpc_lut_smooth alone (LutSmoothFn) reads contrast slots nobody wrote: there only the
SMOOTH scalar means anything, and only it is read here.

Measured on an MI355X (profiles/contrast_cases_runs.md has every output): the largest error-to-bound ratios are 0.27 for the blurred
image, 0.13 / 0.11 for the l2 / variance adjoint image, 0.25 for grad_field, 0.02 to 0.08 for the scalars, 0.55 / 0.78 for the pooling
pair; the l1 adjoint image reaches its bound only under an allowance (at most 1.3 % of a case's pixels have one; 0.11 on the
rest).  213 tests in 4 s; under the bounds-checked build 0 violations."""
import ctypes

import pytest
import torch

import contrast_cases as CC

pytestmark = pytest.mark.gpu

NAMES = ('LOSS', 'FOCUS', 'SMOOTH', 'VAL', 'GCOEF')


def _dev():
    return torch.device('cuda:0')


def _shape(B, nb, T, H, W, sp, flags=0):
    from motionpriorcmax_amd import _lib as C
    return C.Shape(B=B, M=0, Mp=0, nb=nb, T=T, H=H, W=W, sp=sp, hq=-(-H // sp), wq=-(-W // sp), n=0, K=0, flags=flags)


def _ws(shape):
    from motionpriorcmax_amd import ops
    ws = ops.alloc_workspace(shape, _dev())
    ws.fill_(0xFF)
    return ws


def _scalars(scal):
    from motionpriorcmax_amd import _lib as C
    s = scal.cpu()
    return {k: float(s[getattr(C, 'SCAL_' + k)]) for k in NAMES}


def _flags(objective):
    from motionpriorcmax_amd import _lib as C
    return dict(l1=0, l2=C.F_NORM_L2, variance=C.F_OBJ_VARIANCE)[objective]


def _run_images(name, objective, want_grad, with_field):
    """-> blur, gimg, scalars, grad_field of one image case: mpc_lut_smooth (if with_field), mpc_contrast_fwd, mpc_finalize on one
    0xFF-filled workspace."""
    from motionpriorcmax_amd import ops
    raw = CC.image_case(name).to(_dev())
    n, H, W = raw.shape
    shape = _shape(n, 1, 1, H, W, 4, _flags(objective))
    ws = _ws(shape)
    gf = None
    if with_field:
        gf = ops.lut_smooth(shape, CC.image_field(name).to(_dev()), n, 2, CC.SMOOTH_WEIGHT, ws, True)
    blur, gimg = ops.contrast_fwd(shape, raw, ws, want_grad)
    scal = ops.finalize(shape, n if with_field else 0, 2 if with_field else 0, CC.SMOOTH_WEIGHT if with_field else 0.0, ws, _dev())
    return blur, gimg, _scalars(scal), gf


@pytest.mark.parametrize('name,objective', [(n, 'l1') for n in CC.L1_CASES] + [(n, 'l2') for n in CC.L2_CASES])
def test_marching_contrast_vs_float64(name, objective):
    from motionpriorcmax_amd import ops
    r, sm = CC.image_expected(name, objective), CC.field_expected(name)
    if objective == 'l1':
        assert r['share'] <= CC.L1_CAP
    with ops.KernelTimer() as kt:
        blur, gimg, scal, gf = _run_images(name, objective, True, True)
    assert 'k_contrast_march' in kt.summary() and 'k_contrast_fwd' not in kt.summary(), kt.summary()
    label = f'{name} {objective}'
    CC.compare(label, 'blur', blur, r['blur'], r['e_blur'])
    CC.compare(label, f'gimg_{objective}', gimg, r['gimg'], r['e_gimg'])
    if objective == 'l1':
        # (the same check once more on the pixels no ambiguous response reaches, so that their ratio is recorded on its own:
        # a flipped sign under an allowance puts the ratio of the line above near 1)
        clear = r['allow'] == 0
        CC.compare(label, 'gimg_l1_no_allowance', gimg.cpu()[clear], r['gimg'][clear], r['e_gimg'][clear])
    CC.compare(label, 'grad_field', gf, sm['gfield'], sm['e_gfield'])
    CC.compare_scalars(label, scal, CC.scalar_reference(r, sm))


@pytest.mark.parametrize('objective', ['l1', 'l2'])
@pytest.mark.parametrize('name', CC.FWD_CASES)
def test_tiled_forward_only_vs_float64_and_marching(name, objective):
    """want_grad = False: k_contrast_fwd (64 x 32 LDS tiles) -- blur and value; and the value of the marching kernel on the same
    images lies within the sum of the two bounds."""
    from motionpriorcmax_amd import ops
    r = CC.image_expected(name, objective)
    with ops.KernelTimer() as kt:
        blur, gimg, scal, _ = _run_images(name, objective, False, False)
    assert gimg is None and 'k_contrast_fwd' in kt.summary() and 'k_contrast_march' not in kt.summary(), kt.summary()
    want = CC.scalar_reference(r)
    label = f'{name} {objective} forward-only'
    CC.compare(label, 'blur', blur, r['blur'], r['e_blur'])
    CC.compare_scalars(label, scal, want)
    assert scal['SMOOTH'] == 0.0
    _, _, march, _ = _run_images(name, objective, True, False)
    print(f'{label}: VAL tiled {scal["VAL"]!r} marching {march["VAL"]!r} float64 {want["VAL"][0]!r} bound {want["VAL"][1]:.3e}')
    assert abs(scal['VAL'] - march['VAL']) <= 2 * want['VAL'][1]


@pytest.mark.parametrize('want_grad', [True, False])
@pytest.mark.parametrize('name', CC.VAR_CASES)
def test_variance_objective_vs_float64(name, want_grad):
    """k_contrast_fwd, k_image_means, k_contrast_bwd_var; batch b holds the offset image (mean 100, deviation 1)."""
    r = CC.image_expected(name, 'variance')
    blur, gimg, scal, _ = _run_images(name, 'variance', want_grad, False)
    label = f'{name} variance'
    CC.compare(label, 'blur', blur, r['blur'], r['e_blur'])
    if want_grad:
        CC.compare(label, 'gimg_variance', gimg, r['gimg'], r['e_gimg'])
    CC.compare_scalars(label, scal, CC.scalar_reference(r))


@pytest.mark.parametrize('name', CC.FIELD_CASES)
def test_smoothness_vs_float64(name):
    from motionpriorcmax_amd import ops
    d = CC.field_geometry(name)
    r = CC.smooth_expected(name)
    shape = _shape(d['B'], d['nb'], d['T'], d['H'], d['W'], d['sp'])
    assert (shape.hq, shape.wq) == (d['hq'], d['wq'])
    field = CC.field_case(name).to(_dev())
    want = CC.scalar_reference(dict(val=1.0, e_val=0.0, k=1.0), r)['SMOOTH']
    got = {}
    for want_grad in (True, False):
        ws = _ws(shape)
        gf = ops.lut_smooth(shape, field, d['nimg'], d['C'], CC.SMOOTH_WEIGHT, ws, want_grad)
        # (no contrast pass ran: of the scalars only SMOOTH is defined)
        got[want_grad] = _scalars(ops.finalize(shape, d['nimg'], d['C'], CC.SMOOTH_WEIGHT, ws, _dev()))['SMOOTH']
        CC.compare(f'{name} grad={want_grad}', 'SMOOTH', got[want_grad], *want)
        if want_grad:
            CC.compare(name, 'grad_field', gf, r['gfield'], r['e_gfield'])
        else:
            assert gf is None
    assert got[True] == got[False]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _pool_inputs(H, W, n=3):
    g = CC.gen(17 * H + W)
    return torch.randn(n, H, W, generator=g), torch.randn(n, H // 2, W // 2, generator=g)


@pytest.mark.parametrize('shape', CC.POOL_SHAPES)
def test_pool2_forward_and_backward_vs_float64(shape):
    """Odd H and W: the last row / column has no window; it takes no part in the forward and receives nothing in the backward
    (bound 0: its value is unchanged, bit for bit).  Coefficient ratios 0, inf and NaN pass nothing on."""
    from motionpriorcmax_amd import _lib as C
    L = C.lib()
    H, W = shape
    big, small = _pool_inputs(H, W)
    n = big.shape[0]
    dbig, dsmall = big.to(_dev()), small.to(_dev())
    out = torch.full((n, H // 2, W // 2), float('nan'), device=_dev())
    C.check(L.mpc_pool2_fwd(_p(dbig), _p(out), n, H, W, None), 'mpc_pool2_fwd')
    torch.cuda.synchronize()
    CC.compare(f'{H}x{W}', 'pool_fwd', out, *CC.pool_fwd_reference(big))
    for cs, cb in CC.POOL_COEFS:
        acc = dbig.clone()
        dcs, dcb = torch.tensor([cs], device=_dev()), torch.tensor([cb], device=_dev())
        C.check(L.mpc_pool2_bwd_add(_p(dsmall), _p(dcs), _p(acc), _p(dcb), n, H, W, None), 'mpc_pool2_bwd_add')
        torch.cuda.synchronize()
        ref, e = CC.pool_bwd_reference(small, cs, cb, big)
        CC.compare(f'{H}x{W} {cs}/{cb}', 'pool_bwd', acc, ref, e)
        if CC.pool_ratio(cs, cb) == 0.0:
            assert torch.equal(acc, dbig)
        else:
            assert not torch.equal(acc[:, :2 * (H // 2), :2 * (W // 2)], dbig[:, :2 * (H // 2), :2 * (W // 2)])


@pytest.mark.parametrize('count', CC.SCALE_COUNTS)
def test_scale_is_the_fp32_product(count):
    """One rounding per element: equal to torch's fp32 product bit for bit; nothing is written past `count`."""
    from motionpriorcmax_amd import _lib as C
    g = CC.gen(count)
    x = torch.randn(count, generator=g).to(_dev())
    a = torch.tensor([-0.37], device=_dev())
    y = torch.full((count + 64,), 7.0, device=_dev())
    C.check(C.lib().mpc_scale(_p(x), _p(a), _p(y), count, None), 'mpc_scale')
    torch.cuda.synchronize()
    assert torch.equal(y[:count], x * a) and bool((y[count:] == 7.0).all())
