"""The contrast / smoothness cases of tests/contrast_cases.py on the CPU: the float64 reference against float64 autograd through
the oracle's forward (l2, variance, smoothness; l1 where nothing is ambiguous), the tilings the named cases claim to reach, the cap
on the l1 allowance, and the comparator itself -- a float32 torch implementation of every stage passes it on every case, and five
mutants of that implementation fail it with an assertion that names the first bad element."""
import re

import pytest
import torch

import contrast_cases as CC
from oracle import focus_oracle as O


def _autograd_image(raw32, objective):
    raw = raw32.double().requires_grad_(True)
    b = O.gaussian_blur3(raw[:, None])[:, 0]
    val = O.contrast_value(b, 'variance') if objective == 'variance' else O.contrast_value(b, 'gradient_magnitude', objective)
    (1.0 / val).backward()
    return float(val.detach()), raw.grad


# (batch b is ambiguous for l1 by construction and never used with it)
@pytest.mark.parametrize('name,objective', [(n, o) for n in ('3x3b', '4x4b', '17x57b', '33x57b', '47x113b', '16x56a', '32x65a')
                                            for o in ('l2', 'variance', 'l1') if not (o == 'l1' and n[-1] == 'b')])
def test_image_reference_is_the_oracles_gradient(name, objective):
    raw = CC.image_case(name)
    r = CC.image_reference(raw, objective)
    val, grad = _autograd_image(raw, objective)
    assert abs(r['val'] - val) <= 1e-13 * abs(val)
    g = -r['k'] / r['val'] ** 2 * r['gimg']
    # (l1: autograd keeps the sign of a response the reference calls ambiguous; they agree wherever no such response reaches)
    clear = r['allow'] == 0 if objective == 'l1' else torch.ones_like(g, dtype=torch.bool)
    assert float(clear.double().mean()) > 0.9
    assert float(((g - grad).abs() * clear).max()) <= 1e-12 * float(grad.abs().max())
    if objective != 'variance':
        _, g2 = O.contrast_grad_image(raw.double()[:, None], objective)
        assert float(((g - g2[:, 0]).abs() * clear).max()) <= 1e-12 * float(grad.abs().max())
    assert torch.equal(r['blur'], O.gaussian_blur3(raw.double()[:, None])[:, 0])
    M = CC.blur_matrix(raw.shape[-2])
    assert float((M @ raw.double() @ CC.blur_matrix(raw.shape[-1]).t() - r['blur']).abs().max()) <= 1e-14 * float(raw.abs().max())


@pytest.mark.parametrize('name', ['1x1c2t3', '2x3c6t3', '8x61c6n3', '17x61c6t3', '33x2c6n3'])
def test_smooth_reference_is_the_oracles_gradient(name):
    f = CC.field_case(name).double().requires_grad_(True)
    loss = CC.SMOOTH_WEIGHT * O.smoothness(f.permute(0, 3, 1, 2), CC.EPS)
    loss.backward()
    r = CC.smooth_expected(name)
    assert abs(r['smooth'] - float(loss)) <= 1e-14 * abs(float(loss))
    assert float((r['gfield'] - f.grad).abs().max()) <= 1e-12 * float(f.grad.abs().max())


def test_cases_reach_the_tilings_they_claim():
    assert CC.contrast_band(33, 57, 384) == 32 and CC.contrast_band(33, 57, 383) == 16 and CC.contrast_band(33, 57, 1400) == 32
    assert CC.contrast_slots(33, 57, 1400) == 8400 > 8192 and 2 * 2 * 1400 < 8400         # two trips of k_finalize; slots to clear
    assert CC.smooth_band(17, 61, 384, 2) == 16 and CC.smooth_band(17, 61, 383, 2) == 8
    assert CC.smooth_band(17, 61, 128, 6) == 16 and CC.smooth_band(17, 61, 127, 6) == 8
    assert CC.smooth_blocks(2, 3, 2734, 6) == 8202 > 8192
    hs, ws = {s[0] for s in CC.IMG_SHAPES}, {s[1] for s in CC.IMG_SHAPES}
    assert hs == {3, 4, 15, 16, 17, 31, 32, 33, 47} and ws == {3, 4, 55, 56, 57, 59, 60, 61, 63, 64, 65, 113}
    assert {s[0] for s in CC.FIELD_SHAPES} == {1, 2, 7, 8, 9, 15, 16, 17, 33}
    assert {s[1] for s in CC.FIELD_SHAPES} == {1, 2, 3, 59, 60, 61, 62, 121}
    for name in CC.FIELD_CASES:
        d = CC.field_geometry(name)
        assert (d['hq'], d['wq']) == (-(-d['H'] // d['sp']), -(-d['W'] // d['sp'])) and min(d['H'], d['W']) >= 3
        assert d['nimg'] <= d['B'] * d['nb'] and CC.field_case(name).shape == (d['nimg'], d['hq'], d['wq'], d['C'])


@pytest.mark.parametrize('name', CC.L1_CASES)
def test_l1_allowance_cap(name):
    r = CC.image_expected(name, 'l1')
    print(f'{name}: share of pixels with an allowance {r["share"]:.4f}, ambiguous responses {r["ambiguous"]}')
    assert r['share'] <= CC.L1_CAP


def _check_image(name, objective, mutant=None):
    raw = CC.image_case(name)
    r = CC.image_expected(name, objective)
    out = CC.f32_contrast(raw, objective, mutant)
    sm = CC.field_expected(name)
    fs = CC.f32_smooth(CC.image_field(name))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).float())        # noqa: E731
    got = dict(VAL=out['VAL'], FOCUS=out['FOCUS'], GCOEF=out['GCOEF'], SMOOTH=fs['SMOOTH'], LOSS=f32(out['focus64'] + fs['smooth64']))
    label = f'{name} {objective}'
    CC.compare(label, 'blur', out['blur'], r['blur'], r['e_blur'])
    CC.compare(label, f'gimg_{objective}', out['gimg'], r['gimg'], r['e_gimg'])
    CC.compare_scalars(label, got, CC.scalar_reference(r, sm))


@pytest.mark.parametrize('name,objective', [(n, 'l1') for n in CC.L1_CASES] + [(n, 'l2') for n in CC.L2_CASES]
                         + [(n, 'variance') for n in CC.VAR_CASES + CC.FWD_CASES[-1:]])
def test_float32_images_pass(name, objective):
    _check_image(name, objective)


def _check_field(name, mutant=None):
    r = CC.smooth_expected(name)
    out = CC.f32_smooth(CC.field_case(name), mutant=mutant)
    CC.compare(name, 'SMOOTH', out['SMOOTH'], *CC.scalar_reference(dict(val=1.0, e_val=0.0, k=1.0), r)['SMOOTH'])
    CC.compare(name, 'grad_field', out['gfield'], r['gfield'], r['e_gfield'])


@pytest.mark.parametrize('name', CC.FIELD_CASES)
def test_float32_fields_pass(name):
    _check_field(name)


def _pool_inputs(H, W, n=3):
    g = CC.gen(17 * H + W)
    return torch.randn(n, H, W, generator=g), torch.randn(n, H // 2, W // 2, generator=g)


def _check_pool(H, W, cs, cb, mutant=None):
    big, small = _pool_inputs(H, W)
    CC.compare(f'{H}x{W}', 'pool_fwd', CC.f32_pool_fwd(big), *CC.pool_fwd_reference(big))
    CC.compare(f'{H}x{W} {cs}/{cb}', 'pool_bwd', CC.f32_pool_bwd(small, cs, cb, big, mutant), *CC.pool_bwd_reference(small, cs, cb, big))


@pytest.mark.parametrize('coefs', CC.POOL_COEFS)
@pytest.mark.parametrize('shape', CC.POOL_SHAPES)
def test_float32_pool_passes(shape, coefs):
    _check_pool(*shape, *coefs)
    assert (CC.pool_ratio(*coefs) != 0.0) == (coefs in ((-0.5, -2.0), (-3e-3, -7e-5)))


MUTANTS = [('no_fold', lambda: _check_image('17x57a', 'l2', 'no_fold'), 'gimg_l2'),
           ('no_fold', lambda: _check_image('33x57a', 'l1', 'no_fold'), 'gimg_l1'),
           ('col56', lambda: _check_image('17x57a', 'l2', 'col56'), r'blur: first bad element \(\d+, \d+, 56\)'),
           ('col56', lambda: _check_image('33x63a', 'l1', 'col56'), r'blur: first bad element \(\d+, \d+, 56\)'),
           ('stale_slot', lambda: _check_image('slots_1400', 'l2', 'stale_slot'), 'VAL'),
           ('stale_slot', lambda: _check_image('band32_384', 'l1', 'stale_slot'), 'VAL'),
           ('pair_offset', lambda: _check_field('9x61c6t3', 'pair_offset'), 'SMOOTH'),
           ('odd_row', lambda: _check_pool(5, 4, -0.5, -2.0, 'odd_row'), r'pool_bwd: first bad element \(0, 4, 0\)')]


@pytest.mark.parametrize('i', range(len(MUTANTS)))
def test_mutants_fail_the_comparator(i):
    """Reflect fold dropped at row H - 2, column 56 computed with a zero neighbour, one partial-sum slot left stale, channel pair 1
    read at pair 0's offset, odd last row included in the pool: each is caught, by the output it corrupts first."""
    name, run, where = MUTANTS[i]
    with pytest.raises(AssertionError, match='first bad element') as e:
        run()
    assert re.search(where, str(e.value)), str(e.value)


def test_mutants_corrupt_the_elements_they_should():
    """The dropped fold moves row H - 2 of the adjoint image only; the channel-pair mutant leaves pair 0's gradient right."""
    raw = CC.image_case('17x57a')
    r = CC.image_expected('17x57a', 'l2')
    out = CC.f32_contrast(raw, 'l2', 'no_fold')
    bad = ~((out['gimg'].double() - r['gimg']).abs() <= r['e_gimg'])
    assert bool(bad[:, 15].any()) and not bool(bad[:, :15].any()) and not bool(bad[:, 16].any())
    f = CC.smooth_expected('9x61c6t3')
    out = CC.f32_smooth(CC.field_case('9x61c6t3'), mutant='pair_offset')
    bad = ~((out['gfield'].double() - f['gfield']).abs() <= f['e_gfield'])
    assert bool(bad[..., 2:4].any()) and not bool(bad[..., :2].any()) and not bool(bad[..., 4:].any())
