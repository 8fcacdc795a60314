"""The ground-truth flow targets on the host: the fp32 restatement of tests/flow_targets_oracle.py against the g17_targets fixtures
(tools/gen_golden_targets.py: the unmodified reference's loaders, the same formulas in float64 and the distance between the two) and
against torch's own F.interpolate chain at the shipped size, the C ABI of the two new entry points, and the argument errors of
utils.flow_targets, each raised before any GPU call.

Tolerance rule (shared with tests/test_gpu_flow_targets.py): max|out - flow64| <= 2 * err_ref, err_ref = max|flow_ref - flow64| the
reference's own fp32 error (from the fixture, or computed here from torch's result).  The reference and the restatement perform the
same five roundings per element; the factor 2 covers another rounding order, and a wrong tap or weight shows at >= 0.1 of the flow
magnitude, five orders above the bound.  flow_valid and id_mask are held to equality, case d (same size) also on the flow.  Every
figure is printed before it is asserted (pytest -s shows them)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flow_targets_oracle as O
from conftest import ROOT, load_golden

EVIMO2_CASES = ['a', 'b', 'c', 'd']


def load_case(case):
    return load_golden('g17_targets_' + case)


def seeded_raw(B, S, H=480, W=640, share=0.2, seed=17):
    """A seeded [B, S, 2, H, W] block with `share` NaN: blobs over both channels and single-channel NaNs."""
    gen = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, S, 2, H, W, generator=gen) * 5.0
    blob = torch.nn.functional.interpolate((torch.rand(B, S, H // 16, W // 16, generator=gen) < 0.75 * share).float(), size=(H, W), mode='nearest') > 0
    raw[blob[:, :, None].expand_as(raw)] = float('nan')
    raw[torch.rand(B, S, 2, H, W, generator=gen) < 0.15 * share] = float('nan')
    return raw


@pytest.mark.parametrize('case', EVIMO2_CASES)
def test_restatement_matches_the_evimo2_fixtures(case):
    g = load_case(case)
    flow, valid, ids, xs, ys = O.evimo2(g['raw_flow'], tuple(g['out_size']), g['obj_id_mask'])
    assert flow.dtype == np.float32
    O.check_flow(f'{case} restatement', flow, g['flow64'], float(g['err_ref']))
    assert np.array_equal(valid, g['flow_valid']) and np.array_equal(ids, g['id_mask'])
    assert (xs, ys) == (float(g['x_scale']), float(g['y_scale']))
    if case == 'd':
        assert np.array_equal(flow, g['flow']) and np.array_equal(flow, np.where(np.isnan(g['raw_flow']), np.float32(0), g['raw_flow']))
    # the float64 restatement reproduces the fixture's yardstick
    assert np.array_equal(O.evimo2(g['raw_flow'], tuple(g['out_size']), dtype=np.float64)[0], g['flow64'])


def test_restatement_matches_the_multiflow_fixture():
    g = load_case('e')
    for suffix in ('', '_odd'):
        flow = O.multiflow(g['raw_flow' + suffix])
        assert flow.shape == g['flow' + suffix].shape
        O.check_flow(f'e{suffix} restatement', flow, g['flow64' + suffix], float(g['err_ref' + suffix]))
    assert float(g['x_scale']) == float(g['y_scale']) == 0.5


def test_the_fixtures_hold_what_the_cases_are_for():
    a, b, c, d = (load_case(k) for k in EVIMO2_CASES)
    raw = a['raw_flow']
    assert raw.shape == (2, 6, 2, 20, 28) and tuple(a['out_size']) == (16, 24) and a['obj_id_mask'].max() == 255
    assert np.isnan(raw[1, 2]).all() and not np.isnan(raw[0, 4]).any() and (np.isnan(raw[:, :, 0]) ^ np.isnan(raw[:, :, 1])).any()
    for g in (a, b, c, d):
        assert 0.0 < g['flow_valid'].mean() < 1.0 and (float(g['err_ref']) > 0.0) == (g is not d)
    # case b: the nearest tap is neither bilinear neighbour for some rows (at 1.25 it always is i0)
    y0, y1, _ = O.src_half_pixel(21, 13)
    ny = O.src_nearest(21, 13)
    assert ((ny != y0) & (ny != y1)).any() and (ny != y0).any()
    assert (O.src_nearest(20, 16) == O.src_half_pixel(20, 16)[0]).all() and (O.src_nearest(640, 512) == O.src_half_pixel(640, 512)[0]).all()
    assert tuple(c['out_size'])[1] % 4 != 0 and tuple(d['out_size']) == d['raw_flow'].shape[-2:]
    e = load_case('e')
    assert e['raw_flow'].shape == (2, 3, 20, 28, 2) and e['flow'].shape == (2, 3, 2, 10, 14) and e['flow_odd'].shape == (2, 3, 2, 10, 13)


def test_restatement_matches_torch_at_the_shipped_size():
    """480 x 640 -> 384 x 512, B = 1, S = 2, 20 % NaN: torch's own operator chain on the CPU is the reference, err_ref its distance
    to the float64 restatement."""
    raw = seeded_raw(1, 2)
    ids = torch.randint(0, 256, (1, 480, 640), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    assert 0.15 < torch.isnan(raw).float().mean() < 0.3
    ref_flow, ref_valid, ref_ids = O.torch_chain_evimo2(raw, (384, 512), ids)
    flow64 = O.evimo2(raw.numpy(), (384, 512), dtype=np.float64)[0]
    err_ref = float(np.abs(ref_flow.numpy().astype(np.float64) - flow64).max())
    assert err_ref > 0.0
    flow, valid, idm, _, _ = O.evimo2(raw.numpy(), (384, 512), ids.numpy())
    O.check_flow('480x640 -> 384x512 restatement against torch', flow, flow64, err_ref)
    assert np.array_equal(valid, ref_valid.numpy()) and np.array_equal(idm, ref_ids.numpy())


def test_the_header_declares_and_the_library_exports_the_entry_points():
    from motionpriorcmax_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mpcmax.h')).read()
    header = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mpc_flow_targets_supported', 'mpc_flow_targets'):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    m = re.search(r'typedef struct mpc_targets_shape \{([^}]*)\} mpc_targets_shape;', header)
    assert m and [f.strip() for f in m.group(1).replace('int32_t', '').strip(' ;').split(',')] == [k for k, _ in _lib.TargetsShape._fields_]
    assert _lib.lib().mpc_version() == 107 and re.search(r'#define MPC_VERSION 107\b', src)


def test_supported_is_host_only_and_names_what_is_wrong():
    from motionpriorcmax_amd import _lib
    L = _lib.lib()

    def rc(**kw):
        d = dict(B=6, S=6, H=480, W=640, Ho=384, Wo=512, mode=0, has_id=1)
        d.update(kw)
        return L.mpc_flow_targets_supported(ctypes.byref(_lib.TargetsShape(**d)))
    assert rc() == 0 and rc(B=1, S=1, has_id=0) == 0 and rc(mode=1, has_id=0, Ho=240, Wo=320) == 0 and rc(Ho=480, Wo=640) == 0
    for bad in (dict(B=0), dict(mode=1, has_id=0, Ho=1, Wo=320), dict(mode=1, has_id=1, Ho=240, Wo=320)):
        code = rc(**bad)
        assert code < 0, bad
        assert L.mpc_last_error_string().decode().startswith('mpc_flow_targets_supported: '), bad
        assert len(L.mpc_last_error_string()) > len('mpc_flow_targets_supported: '), bad
    assert rc(S=0) < 0 and rc(Wo=0) < 0 and rc(mode=2) < 0
    shape = _lib.TargetsShape(B=1, S=1, H=8, W=8, Ho=4, Wo=4, mode=0, has_id=0)
    assert L.mpc_flow_targets(ctypes.byref(shape), None, None, None, None, None, None) == _lib.E_NULL
    assert L.mpc_flow_targets(None, None, None, None, None, None, None) == _lib.E_NULL


def test_argument_errors_come_before_any_gpu_call():
    """CPU tensors throughout: a ValueError here was raised before anything asked for the device (which raises RuntimeError)."""
    from motionpriorcmax_amd import utils
    f = utils.flow_targets
    raw = torch.zeros(1, 2, 2, 12, 16)
    last = torch.zeros(1, 2, 12, 16, 2)
    for args, kw in (((raw[0], (6, 8)), dict(dataset='evimo2')),                                  # a wrong rank
                     ((raw,), dict(dataset='evimo2')),                                            # no out_size
                     ((last, (6, 9)), dict(dataset='multiflow')),                                 # not (H // 2, W // 2)
                     ((last, (12, 16)), dict(dataset='multiflow')),
                     ((last,), dict(dataset='multiflow', id_mask=torch.zeros(1, 12, 16))),        # MultiFlow has no id mask
                     ((raw, (6, 8)), dict(dataset='dsec')),
                     ((raw.permute(0, 1, 3, 4, 2), (6, 8)), dict(dataset='evimo2')),              # channels in the wrong place
                     ((raw, (6, 8)), dict(dataset='evimo2', id_mask=torch.zeros(1, 6, 8))),       # id mask at the output size
                     ((raw, (0, 8)), dict(dataset='evimo2')),
                     ((torch.zeros(0, 2, 2, 12, 16), (6, 8)), dict(dataset='evimo2'))):
        with pytest.raises(ValueError):
            f(*args, **kw)
    with pytest.raises(TypeError):
        f(raw, (6, 8))                                                                            # dataset is required
    with pytest.raises(RuntimeError):                                                             # CPU tensors raise, as everywhere in the package
        f(raw, (6, 8), dataset='evimo2')
    with pytest.raises(RuntimeError):
        f(last, dataset='multiflow')
