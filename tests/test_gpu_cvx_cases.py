"""The RAFT-spline output head (csrc/cvx_curves.hip, csrc/cvx_device.h) element by element against the references of
tests/cvx_cases.py, through the C entry points themselves (ops._call / ops._query: tile, basis matrix and buffers chosen freely):
fill planes above 1024 cells with a partial last chunk and both store forms, tiles that do not divide 8 (1, 3, 5, 16, 32), a basis
staged in two and three passes, d at both ends of each of the three instantiations, cells without a centre, no centre at all, and
a workgroup that holds the end of one sample and the start of the next.

Exact cases: selector inputs (asserted exact by the case builder), so traj, the flows at every pixel, both gradients and the
workspace's dflow and weights are compared bit for bit with float64.  Every output sits between guard bands and starts as NaN: no
launch writes outside its output or beyond the reported workspace, or leaves an element unwritten.  A gradient asked for alone has the
bits it has beside the other; the public functions give the bits of the raw calls at tiles 2, 4, 8, 16 and launch no k_cvx_* kernel
at tiles 1, 3, 5, 32.  mpc_pec_head_rows / _bwd, which reuse cvx_up and mpc_cvx_traj_bwd, are held to the same references.

Weighted cases, in two stages.  Stage 1: the device's weights of every pixel (a tile-1 backward leaves them in its workspace) against
the float64 softmax per element, relative error at most 4 x the largest such error of the CPU's fp32 torch.softmax on the same
logits (floor 4 * 2^-24): the rule of tests/test_cvx_traj_host.py.  Stage 2: everything after the weights, evaluated in float64 from
the DEVICE's weights, per element |X_gpu - X64| <= gamma(N_X) * A_X with N_X counted in cvx_cases.roundings; no measured number enters,
an element with A_X = 0 has to be exactly 0, and a forward and a backward that disagreed on the weights would fail it.  Every figure is
printed before it is asserted (pytest -s shows them).

Measured on an MI355X (profiles/cvx_cases_runs.md): every exact comparison bit for bit; the weights' largest relative error 6.60 * 2^-24
against the CPU's 6.60 (logits in +-8), at most 1.35 x the CPU's figure on any case; the largest error-to-bound ratio of stage 2 is
0.62 (flows at d = 1, N = 11).  45 tests in 3 s."""
import ctypes

import pytest
import torch

import cvx_cases as CK

pytestmark = pytest.mark.gpu

GUARD = 64                                     # floats on either side of a guarded buffer (a multiple of 4: the buffer stays 16-byte aligned)
SENTINEL = 0x7FC0BEEF                          # a NaN bit pattern no kernel produces
FWD = {'k_cvx_traj_fwd', 'k_cvx_flow_fwd'}


def _dev():
    return torch.device('cuda', 0)


def _launches(kt):
    return {k.split('<')[0]: v['launches'] for k, v in kt.summary().items()}


class _Guarded:
    """`numel` floats of NaN between two bands of SENTINEL.  ptr: the first float (never null, also for numel = 0)."""

    def __init__(self, *shape):
        self.shape = shape
        self.numel = 1
        for v in shape:
            self.numel *= v
        self.buf = torch.full((self.numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=_dev())
        self.buf[GUARD:GUARD + self.numel] = torch.tensor(float('nan')).view(torch.int32)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)
        assert self.ptr.value % 16 == 0

    def take(self, written=None):
        """The guards are untouched and so is everything from `written` floats on; -> the written part on the host, as floats."""
        bits = self.buf.cpu()
        written = self.numel if written is None else written
        assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + self.numel:] == SENTINEL).all()), 'a guard band was written'
        assert bool((bits[GUARD + written:GUARD + self.numel] == torch.tensor(float('nan')).view(torch.int32)).all()), 'written beyond the layout'
        out = bits[GUARD:GUARD + written].view(torch.float32)
        return out.reshape(self.shape) if written == self.numel else out


def _put(t):
    return t.to(_dev()).contiguous()


def _raw(cs, tile=None, traj=True, flows=True, want_params=True, want_mask=True, cotangent=True):
    """The entry points on a case -> traj, flows, grad_params, grad_mask, dflow, weights on the host (None where not asked for),
    each checked for guard bands and for elements left NaN, and the launch counts.  cotangent False: zeros in the place of
    the case's (a call at another tile than the case's, which is after the weights alone)."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    tile = cs.tile if tile is None else tile
    B, d, T, h, w = cs.B, cs.d, cs.T, cs.h, cs.w
    n = CK.tiles(8 * h, tile) * CK.tiles(8 * w, tile)
    p, m, bm = _put(cs.params), _put(cs.mask), _put(cs.basis)
    out = dict(traj=None, flows=None, grad_params=None, grad_mask=None, dflow=None, weights=None)
    with ops.KernelTimer() as kt:
        if traj:
            o_traj = _Guarded(B, T, n, 2)
            ops._call('mpc_cvx_traj_fwd', dev, ops._ptr(p), ops._ptr(m), ops._ptr(bm), float(cs.scale), o_traj.ptr, B, d, T, h, w, tile)
        if flows:
            o_flows = _Guarded(T, B, 2, 8 * h, 8 * w)
            ops._call('mpc_cvx_flow_fwd', dev, ops._ptr(p), ops._ptr(m), ops._ptr(bm), float(cs.scale), o_flows.ptr, B, d, T, h, w)
        if want_params or want_mask:
            gt = _Guarded(B, T, n, 2)                    # (a valid pointer for n = 0 too)
            gt.buf[GUARD:GUARD + gt.numel] = cs.g.reshape(-1).view(torch.int32).to(dev) if cotangent else 0
            nbytes = ops._query('mpc_cvx_traj_bwd_workspace_bytes', dev, B, d, T, h, w, tile)
            assert nbytes % 256 == 0 and nbytes >= B * n * (2 * d + 9) * 4 > nbytes - 256
            o_gp, o_gm, o_ws = _Guarded(B, 2 * d, h, w), _Guarded(B, 576, h, w), _Guarded(nbytes // 4)
            ops._call('mpc_cvx_traj_bwd', dev, gt.ptr, ops._ptr(p), ops._ptr(m), ops._ptr(bm), float(cs.scale), o_gp.ptr if want_params else None,
                      o_gm.ptr if want_mask else None, B, d, T, h, w, tile, o_ws.ptr if want_params else None)
    torch.cuda.synchronize()
    if traj:
        out['traj'] = o_traj.take()
    if flows:
        out['flows'] = o_flows.take()
    if want_params or want_mask:
        out['grad_params'] = o_gp.take(None if want_params else 0)
        out['grad_mask'] = o_gm.take(None if want_mask else 0)
        ws = o_ws.take(B * n * (2 * d + 9) if want_params else 0)
        if want_params:
            out['dflow'], out['weights'] = ws[:B * 2 * d * n].reshape(B, 2 * d, n), ws[B * 2 * d * n:].reshape(B, 9, n)
    for k, v in out.items():
        assert v is None or not bool(torch.isnan(v).any()), f'{cs.name}: {k} holds a NaN'
    return out, _launches(kt)


def _pixel_weights(cs):
    """The device's weights of every pixel, [B, 9, 8, 8, h, w]: what a backward at tile 1 leaves in its workspace."""
    out, _ = _raw(cs, tile=1, traj=False, flows=False, want_mask=False, cotangent=False)
    assert float(out['grad_params'].abs().max()) == 0.0 and float(out['dflow'].abs().max()) == 0.0
    return CK.dense_weights(out['weights'], cs.h, cs.w)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CK.CASES + (CK.LARGE,))
def test_every_element_bit_for_bit(name):
    cs = CK.case(name)
    out, launches = _raw(cs)
    want = {'k_cvx_flow_fwd': 1, 'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1}
    want.update({'k_cvx_traj_fwd': 1} if cs.n else {})
    assert launches == want, launches
    CK.compare_all(name, name, **out)
    # traj - pos is the flow read at the centres (exact inputs: the difference is exact too)
    py, px = cs.pos[:, 0], cs.pos[:, 1]
    at = out['flows'][:, :, :, py, px]                                                                     # [T, B, (x, y), n]
    assert torch.equal(out['traj'] - cs.pos.float()[None, None], torch.stack((at[:, :, 1], at[:, :, 0]), dim=-1).permute(1, 0, 2, 3))
    # the pixel's weights are the centre's weights: the backward at tile 1 against the backward at the case's tile
    if cs.tile != 1 and name != CK.LARGE:
        dense = _pixel_weights(cs)
        assert torch.equal(dense, CK.softmax64(cs.mask).float())
        assert torch.equal(dense[:, :, py % 8, px % 8, py // 8, px // 8], out['weights'])
    # a gradient asked for alone: the same bits, nothing else written
    only, launches = _raw(cs, traj=False, flows=False, want_mask=False)
    assert launches == ({'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1} if cs.n else {'k_cvx_bwd_params': 1}), launches      # (no centre, no fill: no workgroup)
    assert only['grad_mask'].numel() == 0 and all(torch.equal(only[k], out[k]) for k in ('grad_params', 'dflow', 'weights'))
    only, launches = _raw(cs, traj=False, flows=False, want_params=False)
    assert launches == {'k_cvx_bwd_centres': 1}, launches
    assert only['grad_params'].numel() == 0 and only['dflow'] is None and torch.equal(only['grad_mask'], out['grad_mask'])


def test_no_centre_at_all():
    """tile32_none: the workspace query answers an aligned 0, the forward launches nothing and leaves its (empty) output alone, the
    backward writes every element of both gradients as 0."""
    from motionpriorcmax_amd import ops
    cs = CK.case('tile32_none')
    assert cs.n == 0 and ops._query('mpc_cvx_traj_bwd_workspace_bytes', _dev(), cs.B, cs.d, cs.T, cs.h, cs.w, cs.tile) == 0
    out, launches = _raw(cs, flows=False)
    assert not FWD & set(launches) and launches == {'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1}, launches
    assert out['traj'].numel() == 0 and out['dflow'].numel() == 0 == out['weights'].numel()
    for k in ('grad_params', 'grad_mask'):
        assert out[k].numel() > 0 and torch.equal(out[k], torch.zeros_like(out[k]))
    # the public functions at a kernel tile without a centre (8 w = tile / 2): an empty result and two zero gradients
    from motionpriorcmax_amd import utils
    p, m = _put(cs.params[:, :, :, :1]).requires_grad_(True), _put(cs.mask[:, :, :, :1]).requires_grad_(True)
    with ops.KernelTimer() as kt:
        traj, pos = utils.trajectories_from_bezier(p, torch.tensor(CK.TIMES), 16, (8 * cs.h, 8), scale=cs.scale, up_mask=m)
        assert type(traj.grad_fn).__name__.startswith('CvxCurveTrajFn') and tuple(traj.shape) == (cs.B, 8, 0, 2) and pos.shape[0] == 0
        gp, gm = torch.autograd.grad(traj, [p, m], torch.zeros_like(traj))
    assert not any(k.startswith('k_cvx') for k in _launches(kt))
    assert gp.shape == p.shape and gm.shape == m.shape and float(gp.abs().max()) == 0.0 == float(gm.abs().max())


PUBLIC_KERNEL = ('tile2', 'onehot_border', 'tile8', 'tile16_d16')            # tiles 2, 4, 8, 16
PUBLIC_MIRROR = ('tile1_row', 'tile3', 'tile5_d11', 'tile32_one')            # tiles 1, 3, 5, 32


def _public(cs, p, m):
    from motionpriorcmax_amd import ops, utils
    times = torch.tensor(CK.TIMES, dtype=torch.float64)
    with ops.KernelTimer() as kt:
        traj, pos = utils.trajectories_from_bezier(p, times, cs.tile, (8 * cs.h, 8 * cs.w), scale=cs.scale, up_mask=m)
        gp, gm = torch.autograd.grad(traj, [p, m], _put(cs.g))
        flows = utils.flows_from_bezier(p.detach(), times, up_mask=m.detach(), scale=cs.scale)
    assert torch.equal(pos, cs.pos)
    return traj.detach().cpu(), flows.cpu(), gp.cpu(), gm.cpu(), _launches(kt)


@pytest.mark.parametrize('name', PUBLIC_KERNEL)
def test_the_public_route_has_the_bits_of_the_raw_calls(name):
    cs = CK.with_matrix(name)
    assert cs.tile in (2, 4, 8, 16) and cs.T == 8
    raw, _ = _raw(cs)
    traj, flows, gp, gm, launches = _public(cs, _put(cs.params).requires_grad_(True), _put(cs.mask).requires_grad_(True))
    assert launches == {'k_cvx_traj_fwd': 1, 'k_cvx_bwd_centres': 1, 'k_cvx_bwd_params': 1, 'k_cvx_flow_fwd': 1}, launches
    for k, v in (('traj', traj), ('flows', flows), ('grad_params', gp), ('grad_mask', gm)):
        CK.compare(f'{cs.name} public', k, v, raw[k])


@pytest.mark.parametrize('name', PUBLIC_MIRROR)
def test_other_tiles_take_the_mirror_which_agrees_with_the_node(name):
    """Tiles 1, 3, 5, 32: utils.trajectories_from_bezier launches no k_cvx_* kernel.  The mirror and ops.CvxCurveTrajFn.apply on the
    same inputs under the Bernstein matrix are each held to the rule of stage 2 -- the selector weights are exact on both routes
    (asserted for the node), and the mirror's autograd makes no more roundings on any path than the kernels: the forward has the same
    sums, the backward the same T + 1 for dflow, the same softmax adjoint, and for params the same non-zero terms per cell in some
    other order (adding a zero is exact) -- so the two agree within twice that bound."""
    from motionpriorcmax_amd import ops
    cs = CK.with_matrix(name)
    assert cs.tile in (1, 3, 5, 32)
    traj, flows, gp, gm, launches = _public(cs, _put(cs.params).requires_grad_(True), _put(cs.mask).requires_grad_(True))
    assert set(launches) == {'k_cvx_flow_fwd'}, launches
    p, m = _put(cs.params).requires_grad_(True), _put(cs.mask).requires_grad_(True)
    node = ops.CvxCurveTrajFn.apply(p, m, _put(cs.basis), float(cs.scale), cs.tile)
    ngp, ngm = torch.autograd.grad(node, [p, m], _put(cs.g))
    raw, _ = _raw(cs, flows=False)
    assert torch.equal(raw['weights'].double(), CK.evaluate(cs).weights)
    bounds = CK.stage2_bounds(cs, CK.softmax64(cs.mask))
    for route, outs in (('mirror', dict(traj=traj, grad_params=gp, grad_mask=gm)), ('node', dict(traj=node.detach().cpu(), grad_params=ngp.cpu(), grad_mask=ngm.cpu()))):
        for k, v in outs.items():
            CK.compare(f'{cs.name} {route}', k, v, *bounds[k])
    assert torch.equal(node.detach().cpu(), raw['traj']) and torch.equal(ngp.cpu(), raw['grad_params']) and torch.equal(ngm.cpu(), raw['grad_mask'])


# ---- mpc_pec_head_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CK.HEAD_ROWS_CASES)
def test_head_rows_and_their_adjoint_bit_for_bit(name):
    """rows = scale * up at the centres ((y, x) halves), and mpc_pec_head_rows_bwd -- mpc_cvx_traj_bwd with the identity as its
    matrix behind a transpose of the cotangent -- gives the float64 gradients, every element of both written."""
    from motionpriorcmax_amd import ops
    dev = _dev()
    cs, e, rows, g_rows = CK.head_rows_case(name)
    B, d, h, w, n = cs.B, cs.d, cs.h, cs.w, cs.n
    assert (8 * h) % cs.tile == 0 == (8 * w) % cs.tile and n == (8 * h // cs.tile) * (8 * w // cs.tile)
    p, m = _put(cs.params), _put(cs.mask)
    o_rows, o_gp, o_gm = _Guarded(B * n, 2 * d), _Guarded(B, 2 * d, h, w), _Guarded(B, 576, h, w)
    ops._call('mpc_pec_head_rows', dev, ops._ptr(p), ops._ptr(m), float(cs.scale), cs.tile, o_rows.ptr, B, d, h, w)
    nbytes = ops._query('mpc_pec_head_rows_bwd_workspace_bytes', dev, B, d, h, w, cs.tile)
    ws = _Guarded(nbytes // 4)
    ops._call('mpc_pec_head_rows_bwd', dev, ops._ptr(_put(g_rows)), ops._ptr(p), ops._ptr(m), float(cs.scale), cs.tile, o_gp.ptr, o_gm.ptr, B, d, h, w, ws.ptr)
    torch.cuda.synchronize()
    ws.take()
    CK.compare(cs.name, 'rows', o_rows.take(), rows)
    CK.compare(cs.name, 'grad_params', o_gp.take(), e.grad_params)
    CK.compare(cs.name, 'grad_mask', o_gm.take(), e.grad_mask)
    assert float(rows.abs().max()) > 0 and float(e.grad_params.abs().max()) > 0


# ---- weighted cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', CK.WEIGHTED_VARIANTS)
@pytest.mark.parametrize('shape', list(CK.WEIGHTED_SHAPES))
def test_weighted_in_two_stages(shape, variant):
    cs = CK.weighted(shape, variant)
    # stage 1: the weights of every pixel
    dense = _pixel_weights(cs)
    cpu = CK.weight_error(torch.softmax(cs.mask.reshape(cs.B, 9, 8, 8, cs.h, cs.w), dim=1), cs.mask)
    got = CK.weight_error(dense, cs.mask)
    tol = 4.0 * max(cpu, CK.U)
    print(f'{cs.name}: largest relative error of the weights, device {got / CK.U:.2f} * 2^-24, CPU fp32 softmax {cpu / CK.U:.2f} * 2^-24, '
          f'tolerance {tol / CK.U:.2f} * 2^-24', flush=True)
    assert got <= tol, (cs.name, got, tol)
    # stage 2: everything after them, from the device's weights
    out, _ = _raw(cs)
    py, px = cs.pos[:, 0], cs.pos[:, 1]
    assert torch.equal(dense[:, :, py % 8, px % 8, py // 8, px // 8], out['weights'])
    bounds = CK.stage2_bounds(cs, dense)
    N = CK.roundings(cs)
    for k in ('flows', 'traj', 'dflow', 'grad_mask', 'grad_params'):
        ratio = CK.compare(f'{cs.name} N = {N[k]}', k, out[k], *bounds[k])
        assert ratio <= 1.0
        zero = bounds[k][1] == 0
        assert not bool(zero.any()) or float(out[k][zero].abs().max()) == 0.0

