"""The KNN flow LUT (csrc/knn.hip, knn_strip.hip, knn_device.h) per element and per neighbour against the reference of
tests/knn_cases.py, through the stage entry points mpc_knn_lut_fwd / mpc_knn_lut_bwd (ops.knn_lut_fwd, ops.knn_lut_bwd), and for one
case per route through ops.KnnLutFn.

Per case: the workspace is filled with 0xFF and every output with NaN before the first call; the saved state (K-th distance bit for
bit, K-th index, tie flag, 'iwd' normaliser, per-class tile maxima), flow_lut, flow_next and grad_traj are held to the counted
allowances of knn_cases.py with no element excused (a point that is nobody's neighbour: exactly zero); ops.knn_indices must return
the reference's ordered lists; then ANOTHER case runs in the same workspace and this one again, without refilling, and must give the
same bits (stale lists, counters that nobody zeroes).  Every case also asserts the route it was written for -- kernel launches from
ops.KernelTimer, the fallback list with its reasons, the retry / far-strip lists, the tail launch's counters, KNN_FAR_FLAG bits --
and prints what it saw (pytest -s); profiles/knn_cases_runs.md has the figures of an MI355X."""
import ctypes
import operator

import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu

OPS = {'>': operator.gt, '>=': operator.ge, '==': operator.eq, '<=': operator.le, '<': operator.lt}
NAMES = list(KC.CASES)


def _dev():
    return torch.device('cuda:0')


def _cfg(c):
    from motionpriorcmax_amd import ops
    return ops.PathConfig(image_shape=(c.H, c.W), num_tref=c.T, num_bins=c.nb, num_knn=c.K, smooth_weight=1.0 if c.want_next else 0.0,
                          sp=c.sp, norm_l2=False, dist_l1=(c.norm == 'l1'), scale_by_dt=False, mask_border=False, polarity_split=False,
                          scheme_iwd=(c.scheme == 'iwd'), smooth_on_next=c.want_next)


def _shape(c):
    from motionpriorcmax_amd import ops
    return ops.make_shape(_cfg(c), c.B, 0, 0, c.n)


def _ws_bytes(c):
    from motionpriorcmax_amd import ops
    return max(ops._query('mpc_workspace_bytes', _dev(), ctypes.byref(_shape(c))), 256)


def _i32(ws, off):
    return int(ws[off:off + 4].view(torch.int32).item())


def _counters(c, shape, ws):
    """The work lists the forward left in the workspace (mpcmax.h: mpc_knn_fail_list_offset, mpc_knn_list_offsets,
    mpc_knn_tail_counters_offset)."""
    from motionpriorcmax_amd import _lib as C
    lib = C.lib()
    out = {}
    off = lib.mpc_knn_fail_list_offset(ctypes.byref(shape))
    n = _i32(ws, off)
    assert 0 <= n <= c.B * c.nb * c.hq * c.wq, n
    ent = ws[off + 4:off + 4 + 4 * n].view(torch.int32).cpu()
    out['fails'] = n
    for why in range(4):
        out[f'why{why}'] = int((((ent >> 30) & 3) == why).sum())
    lo = (ctypes.c_int64 * 6)()
    assert lib.mpc_knn_list_offsets(ctypes.byref(shape), lo) == 0
    out['retry'], out['farstrip'] = _i32(ws, lo[0]), _i32(ws, lo[1])
    off = lib.mpc_knn_tail_counters_offset(ctypes.byref(shape))
    out['marked'], out['late'], out['done'] = _i32(ws, off), _i32(ws, off + 128), _i32(ws, off + 256)
    return out


def _run(c, ws, fill, api):
    """Forward and backward of `c` in the workspace `ws` -> outputs (on the host), launches and counters.  api: through ops.knn_lut_fwd /
    ops.knn_lut_bwd as they are; else the same two library calls on outputs filled with NaN beforehand."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    cfg, shape = _cfg(c), _shape(c)
    traj = c.traj.to(dev)
    g_lut, g_next = (None if g is None else g.to(dev) for g in c.cotangents())
    if fill:
        ws.fill_(0xFF)
    with ops.KernelTimer() as kt:
        if api:
            lut, nxt, state, _ = ops.knn_lut_fwd(cfg, shape, traj, ws)
        else:
            nan = float('nan')
            lut = torch.full((c.B, c.nb, c.hq, c.wq, c.T, 2), nan, device=dev)
            nxt = torch.full((c.B, c.nb - 1, c.hq, c.wq, 1, 2), nan, device=dev) if c.want_next else None
            state = torch.full((ops._query('mpc_knn_state_floats', dev, ctypes.byref(shape)),), nan, device=dev)
            ops._call('mpc_knn_lut_fwd', dev, ctypes.byref(shape), ops._ptr(traj), ops._ptr(lut), ops._ptr(nxt), ops._ptr(state), None, ops._ptr(ws))
        torch.cuda.synchronize()
        counters = _counters(c, shape, ws) if KC.strip_usable(c) else {}          # (the lists of the strip kernel and its tail launch)
        if api:
            grad = ops.knn_lut_bwd(shape, traj, g_lut, g_next, state, ws)
        else:
            grad = torch.full_like(traj, float('nan'))
            ops._call('mpc_knn_lut_bwd', dev, ctypes.byref(shape), ops._ptr(traj), ops._ptr(g_lut), ops._ptr(g_next), ops._ptr(state), ops._ptr(grad), ops._ptr(ws))
    seen = {k: v['launches'] for k, v in kt.summary().items()}
    return dict(lut=lut.cpu(), nxt=None if nxt is None or not c.has_next else nxt.cpu(), state=state.cpu(), grad=grad.cpu(), seen=seen, counters=counters)


def _routes(c, r, far_flags, tie_flags):
    ref = KC.reference(c)
    got = dict(r['counters'])
    for k in ('k_knn_strip', 'k_knn_tail', 'k_knn_query', 'k_knn_bucket', 'k_knn_bucket_count', 'k_knn_sat', 'k_knn_bwd_tile', 'k_knn_bwd_far',
              'k_knn_bwd_points', 'k_knn_bwd_combine', 'k_knn_bwd_combine_bins', 'k_knn_bwd_combine_direct'):
        got[k] = r['seen'].get(k, 0)
    got.update(far_flags=far_flags, tie_flags=tie_flags, ref_ties=int(ref['tie'].sum()))
    print(f'{c.name} ROUTE ' + ' '.join(f'{k}={v}' for k, v in got.items() if v), flush=True)
    assert c.expect, c.name
    for key, op, val in c.expect:
        assert OPS[op](got[key], val), f'{c.name}: route not reached: {key} = {got[key]}, written for {op} {val}; saw {got}'


def _same_bits(c, a, b, what):
    sa, sb = KC.split_state(c, a['state']), KC.split_state(c, b['state'])
    pairs = [('flow_lut', a['lut'], b['lut']), ('grad_traj', a['grad'], b['grad']), ('kth distance', sa[0], sb[0]), ('kth index', sa[1], sb[1]),
             ('tile maxima', sa[3], sb[3])]
    if c.has_next:
        pairs.append(('flow_next', a['nxt'], b['nxt']))
    if c.iwd:
        pairs.append(('normaliser', sa[2], sb[2]))
    for name, x, y in pairs:
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), f'{c.name}: {name} differs in bits {what}'


def _device(fn, *args, **kw):
    """A device error ends the session: nothing more is started on a GPU that has faulted."""
    try:
        return fn(*args, **kw)
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'hipError' in str(e) or 'illegal memory access' in str(e):
            pytest.exit(f'device error, session ended: {e}', returncode=3)
        raise


@pytest.mark.parametrize('name', NAMES)
def test_case(name):
    from motionpriorcmax_amd import ops
    c = KC.case(name)
    other = KC.case(NAMES[(NAMES.index(name) + 7) % len(NAMES)])          # (seven on: another family of cases, another shape)
    ws = torch.empty(max(_ws_bytes(c), _ws_bytes(other)), dtype=torch.uint8, device=_dev())
    first = _device(_run, c, ws, fill=True, api=False)
    idx = _device(lambda: ops.knn_indices(_cfg(c), c.traj.to(_dev())).cpu())
    _device(_run, other, ws, fill=False, api=True)
    again = _device(_run, c, ws, fill=False, api=True)
    failed = []          # every assertion of the case is made, so that one run shows all its figures

    def hold(fn, *args):
        try:
            return fn(*args)
        except AssertionError as e:
            failed.append(str(e))

    hold(KC.check_state, c, 'device', first['state'])
    _, ikw, _, _ = KC.split_state(c, first['state'])
    hold(_routes, c, first, int(((ikw & KC.KNN_FAR_FLAG) != 0).sum()), int(((ikw & KC.KNN_TIE_FLAG) != 0).sum()))
    hold(KC.check_forward, c, 'device', first['lut'], first['nxt'])
    hold(KC.check_backward, c, 'device', first['grad'])
    hold(KC.check_indices, c, 'device', idx)
    hold(_same_bits, c, first, again, f'after {other.name} ran in the same workspace')
    if again['counters'] != first['counters']:
        failed.append(f'{c.name}: the work lists differ after {other.name} ran in the same workspace: {first["counters"]} then {again["counters"]}')
    assert not failed, '\n'.join(failed)


@pytest.mark.parametrize('name', KC.FN_CASES)
def test_autograd_function(name):
    from motionpriorcmax_amd import ops
    c = KC.case(name)
    td = c.traj.to(_dev()).requires_grad_(True)
    lut, nxt = _device(ops.KnnLutFn.apply, td, _cfg(c))
    g_lut, g_next = c.cotangents()
    loss = (lut * g_lut.to(_dev())).sum()
    if c.has_next:
        loss = loss + (nxt * g_next.to(_dev())).sum()
    loss.backward()
    KC.check_forward(c, 'KnnLutFn', lut.detach().cpu(), nxt.detach().cpu() if c.has_next else None)
    KC.check_backward(c, 'KnnLutFn', td.grad.cpu())
