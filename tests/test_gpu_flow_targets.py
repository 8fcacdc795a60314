"""The ground-truth flow targets on the device: utils.flow_targets (csrc/flow_targets.hip: mpc_flow_targets) against the g17_targets
fixtures of the unmodified reference (tools/gen_golden_targets.py), against torch's own operator chain at the shipped size, and fed
into utils.trajectory_val_metrics.  The rule of tests/test_flow_targets_host.py: max|out - flow64| <= 2 * err_ref for the flow,
equality for flow_valid and id_mask (and for the flow of case d).  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import flow_targets_oracle as O
import val_metrics_oracle as VO
from test_flow_targets_host import EVIMO2_CASES, load_case, seeded_raw

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _call(g, **kw):
    from motionpriorcmax_amd import utils
    return utils.flow_targets(_t(g['raw_flow']), tuple(int(v) for v in g['out_size']), dataset='evimo2', id_mask=_t(g['obj_id_mask']), **kw)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('case', EVIMO2_CASES)
def test_evimo2_fixtures(case):
    from motionpriorcmax_amd import ops
    g = load_case(case)
    with ops.KernelTimer() as kt:
        out = _call(g)
    launches = {k: v['launches'] for k, v in kt.summary().items()}
    Wo = int(g['out_size'][1])
    assert launches == {('k_flow_targets_vec' if Wo % 4 == 0 else 'k_flow_targets_elem'): 1}, launches          # one launch; a: float4, c: by the element
    flow, valid, ids = out['flow'], out['flow_valid'], out['id_mask']
    assert flow.is_cuda and flow.dtype == torch.float32 and flow.shape == g['flow'].shape and flow.is_contiguous()
    assert valid.dtype == torch.bool and ids.dtype == torch.float32
    O.check_flow(f'{case} gpu', flow.cpu().numpy(), g['flow64'], float(g['err_ref']))
    assert np.array_equal(valid.cpu().numpy(), g['flow_valid']) and np.array_equal(ids.cpu().numpy(), g['id_mask'])
    assert (out['x_scale'], out['y_scale']) == (float(g['x_scale']), float(g['y_scale']))
    if case == 'd':
        assert torch.equal(flow, _t(g['flow'])) and torch.equal(flow, torch.nan_to_num(_t(g['raw_flow']), nan=0.0))


def test_multiflow_fixture():
    from motionpriorcmax_amd import ops, utils
    g = load_case('e')
    for suffix in ('', '_odd'):
        raw = _t(g['raw_flow' + suffix])
        with ops.KernelTimer() as kt:
            out = utils.flow_targets(raw, dataset='multiflow')
        assert sum(v['launches'] for v in kt.summary().values()) == 1
        assert out['flow_valid'] is None and out['id_mask'] is None and (out['x_scale'], out['y_scale']) == (0.5, 0.5)
        O.check_flow(f'e{suffix} gpu', out['flow'].cpu().numpy(), g['flow64' + suffix], float(g['err_ref' + suffix]))
        H, W = raw.shape[2:4]
        _same(out, utils.flow_targets(raw, (H // 2, W // 2), dataset='multiflow'))
    raw = _t(g['raw_flow']).clone()
    raw[0, 1, 4, 6, 0] = float('nan')                                         # a NaN propagates into the pixels that blend it, as in the reference
    nan = torch.isnan(utils.flow_targets(raw, dataset='multiflow')['flow'])
    assert nan[0, 1, 0].any() and not nan[0, 1, 1].any() and not nan[1].any() and int(nan.sum()) <= 4


def test_the_shipped_size_against_torch():
    """480 x 640 -> 384 x 512, B = 2, S = 6, seeded NaN blobs and single-channel NaNs: torch's CPU chain is the reference and err_ref
    its distance to the float64 restatement."""
    from motionpriorcmax_amd import utils
    raw = seeded_raw(2, 6)
    ids = torch.randint(0, 256, (2, 480, 640), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    assert (torch.isnan(raw[:, :, 0]) ^ torch.isnan(raw[:, :, 1])).any()
    ref_flow, ref_valid, ref_ids = O.torch_chain_evimo2(raw, (384, 512), ids)
    flow64 = O.evimo2(raw.numpy(), (384, 512), dtype=np.float64)[0]
    err_ref = float(np.abs(ref_flow.numpy().astype(np.float64) - flow64).max())
    assert err_ref > 0.0
    out = utils.flow_targets(raw.to(_dev()), (384, 512), dataset='evimo2', id_mask=ids.to(_dev()))          # (uint8 ids: converted with torch)
    O.check_flow('480x640 -> 384x512 gpu against torch', out['flow'].cpu().numpy(), flow64, err_ref)
    assert torch.equal(out['flow_valid'].cpu(), ref_valid) and torch.equal(out['id_mask'].cpu(), ref_ids)
    assert (out['x_scale'], out['y_scale']) == (0.8, 0.8)


@pytest.mark.parametrize('case', ['a', 'c'])
def test_a_view_one_float_off_a_16_byte_boundary_and_a_second_call_give_the_same_bits(case):
    from motionpriorcmax_amd import utils
    g = load_case(case)
    raw, ids, size = _t(g['raw_flow']), _t(g['obj_id_mask']), tuple(int(v) for v in g['out_size'])
    a = utils.flow_targets(raw, size, dataset='evimo2', id_mask=ids)
    _same(a, utils.flow_targets(raw, size, dataset='evimo2', id_mask=ids))
    buf = torch.empty(raw.numel() + 1, dtype=torch.float32, device=_dev())
    buf[1:] = raw.flatten()
    view = buf[1:].view(raw.shape)
    assert raw.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    _same(a, utils.flow_targets(view, size, dataset='evimo2', id_mask=ids))


def test_one_image_no_id_mask_and_an_odd_number_of_images():
    """Every pixel is computed on its own: a slice of the batch gives the slice of the result, bit for bit."""
    from motionpriorcmax_amd import utils
    for case in ('a', 'c'):
        g = load_case(case)
        raw, size = _t(g['raw_flow']), tuple(int(v) for v in g['out_size'])
        full = _call(g)
        one = utils.flow_targets(raw[:1, :1].contiguous(), size, dataset='evimo2')
        assert one['id_mask'] is None and one['flow'].shape[:2] == (1, 1)
        assert torch.equal(one['flow'], full['flow'][:1, :1]) and torch.equal(one['flow_valid'], full['flow_valid'][:1, :1])
    g = load_case('a')
    odd = utils.flow_targets(_t(g['raw_flow'])[:1, :5].contiguous(), (16, 24), dataset='evimo2', id_mask=_t(g['obj_id_mask'])[:1])          # B * S = 5
    full = _call(g)
    assert torch.equal(odd['flow'], full['flow'][:1, :5]) and torch.equal(odd['flow_valid'], full['flow_valid'][:1, :5])
    assert torch.equal(odd['id_mask'], full['id_mask'][:1])
    assert load_case('c')['raw_flow'].shape[:2] == (3, 1)                      # (case c itself: B * S = 3, checked against the fixture above)


def test_other_dtypes_are_converted_and_cpu_tensors_raise():
    from motionpriorcmax_amd import utils
    g = load_case('b')
    a = _call(g)
    b = utils.flow_targets(_t(g['raw_flow']).double(), (13, 32), dataset='evimo2', id_mask=_t(g['obj_id_mask']).long())
    _same(a, b)
    with pytest.raises(RuntimeError):
        utils.flow_targets(torch.from_numpy(g['raw_flow']), (13, 32), dataset='evimo2')


def test_no_host_synchronisation():
    g = load_case('a')
    raw, ids = _t(g['raw_flow']), _t(g['obj_id_mask'])
    from motionpriorcmax_amd import utils
    eager = utils.flow_targets(raw, (16, 24), dataset='evimo2', id_mask=ids)          # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = utils.flow_targets(raw, (16, 24), dataset='evimo2', id_mask=ids)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    _same(out, eager)


def test_capture_and_replay_give_the_eager_result():
    """One stream, one kernel node: captured and replayed twice."""
    from motionpriorcmax_amd import utils
    g = load_case('a')
    raw, ids = _t(g['raw_flow']), _t(g['obj_id_mask'])
    eager = utils.flow_targets(raw, (16, 24), dataset='evimo2', id_mask=ids)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                  # warm-up outside the capture
        for _ in range(2):
            utils.flow_targets(raw, (16, 24), dataset='evimo2', id_mask=ids)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = utils.flow_targets(raw, (16, 24), dataset='evimo2', id_mask=ids)
    for _ in range(2):
        for k in ('flow', 'flow_valid', 'id_mask'):
            static[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(static, eager)


def test_the_targets_feed_the_validation_metrics():
    """trajectory_val_metrics on the library's targets and on the reference's targets of case a, the same seeded predictions: every
    `updated` flag equal and every value within the metric rule of tests/test_gpu_val_metrics.py, bound(x, err) = max(4 err,
    2^-22 |x|).  err is what the targets' distance can move a metric by: the two flows lie within 2 err_ref and err_ref of flow64,
    so a ground-truth vector moves by at most d = sqrt(2) * 3 err_ref; |P - G| is 1-Lipschitz in G (the pixel metrics: err = d) and
    the angle between (P, 1) and (G, 1) moves by at most d radians since |(G, 1)| >= 1 (the angle metrics, in degrees: err =
    d * 180 / pi).  The masks are equal, and the seeded predictions keep every pixel off the count thresholds by more than d."""
    from motionpriorcmax_amd import utils
    g = load_case('a')
    out = _call(g)
    gt_ref, valid_ref = _t(g['flow']), _t(g['flow_valid'])
    assert torch.equal(out['flow_valid'], valid_ref)
    B, M, _, H, W = gt_ref.shape
    gen = torch.Generator().manual_seed(172)                                   # (a seed whose predictions pass the margin assertion below)
    mag = torch.exp(torch.rand(M, B, H, W, generator=gen) * (np.log(6.0) - np.log(0.02)) + np.log(0.02))
    ang = torch.rand(M, B, H, W, generator=gen) * (2 * np.pi)
    flows = (torch.from_numpy(g['flow']).permute(1, 0, 2, 3, 4) + torch.stack((mag * torch.cos(ang), mag * torch.sin(ang)), dim=2)).to(_dev())
    em = (torch.rand(B, H, W, generator=gen) < 0.6).to(_dev())
    times = np.arange(1, M + 1) / M
    d = np.sqrt(2.0) * 3.0 * float(g['err_ref'])
    e = (flows.permute(1, 0, 2, 3, 4) - gt_ref).norm(dim=2).double()
    rel = e / gt_ref.norm(dim=2).double().clamp_min(1e-6)
    off = min(float((e - k).abs().min()) for k in (1.0, 2.0, 3.0))
    assert off > 4 * d and float((rel - 0.05).abs()[e > 1.0 - 4 * d].min()) > 1e-3, (off, d)          # (the relative threshold counts only beside e > k)
    lib_v, lib_u = utils.trajectory_val_metrics(out['flow'], times, flows=flows, flow_valid=out['flow_valid'], event_mask=em)
    ref_v, ref_u = utils.trajectory_val_metrics(gt_ref, times, flows=flows, flow_valid=valid_ref, event_mask=em)
    assert list(lib_v) == list(ref_v) and len(lib_v) == 45
    for k in ref_v:
        x, y = ref_v[k].item(), lib_v[k].item()
        err = d * (180.0 / np.pi if ('ae' in k.split('/')[-1].lower()) else 1.0)
        print(f'{k}: {y!r} vs {x!r}  |diff| {abs(y - x):.3g} (bound {VO.bound(x, err):.3g})  updated {lib_u[k].item()} vs {ref_u[k].item()}')
        assert lib_u[k].item() == ref_u[k].item(), k
        if np.isnan(x):
            assert np.isnan(y), k
        else:
            assert abs(y - x) <= VO.bound(x, err), (k, y, x)
