"""The DSEC event ingest (csrc/ingest.hip) per element against the numpy oracle at its edges: the named cases of
tests/ingest_cases.py through `utils.ingest_events` (plain and ordered route, float and rectification-map source), and through
the raw ABI into memory that is known to be dirty.  Every comparison is bit for bit; nothing is skipped and nothing has a
tolerance.  tests/test_ingest_cases_host.py shows on the CPU that every case reaches the edge it names.

UNPINNED (reference src/loader/dsec/loader.py:152-167 pins neither, the oracle and the kernels agree): an event whose polarity
is NaN, or any value other than 0 and 1, is in neither block; a coordinate of +inf or NaN fails the in-image filter."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ingest_cases as IC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a, unaligned=False):
    """`a` on the device; unaligned: as a contiguous view that starts one element into a flat buffer (off 16-byte alignment)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not unaligned:
        return t.to(DEV)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    flat[1:] = t.reshape(-1).to(DEV)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and flat.data_ptr() % 16 == 0
    return v


@functools.lru_cache(maxsize=None)
def _loss(H, W, nb, sp):
    from motionpriorcmax_amd import LossFactory
    cfg = dict(image_shape=(H, W), num_tref=1, num_bins=nb, num_knn=32, smooth_weight=0.003, lut_superpixel_size=sp,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _loss_of(c):
    return _loss(c.H, c.W, c.nb, c.sp)


def _inputs(c, gathered=False):
    x, y, t, p, counts = c.raw()
    if gathered:
        x, y = c.gathered()
    return tuple(_dev(a, c.unaligned) for a in (x, y, t, p)), counts


def _ingest(c, ordered=False, voxel=False, gathered=False):
    from motionpriorcmax_amd.utils import ingest_events
    args, counts = _inputs(c, gathered)
    kw = {'rectify_map': _dev(c.rect_map)} if c.rect_map is not None and not gathered else {}
    return ingest_events(*args, torch.from_numpy(counts), (c.H, c.W), c.nb, want_voxel_input=voxel,
                         order_for=_loss_of(c) if ordered else None, **kw)


def _assert_bits(got, want, nan, what):
    """Equal element for element, NaN where the oracle has NaN (and only in a case that says it has any), and the sign of
    every other element too: -0.0 is not 0.0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not nan:
        assert not np.isnan(want).any() and not np.isnan(got).any(), what
    np.testing.assert_array_equal(got, want, err_msg=str(what))          # (NaN equals NaN here)
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got)[ok], np.signbit(want)[ok]), what


def _assert_xytp(c, xytp, name, tail=None):
    """xytp[b, :n] against the oracle for every sample; `tail`: what the rows behind n must still hold (the raw ABI test's fill)."""
    want = IC.expected(name)[2]
    got = xytp.cpu().numpy()
    assert got.shape == (c.B, c.N, 4)
    for b in range(c.B):
        n = c.n(b)
        _assert_bits(got[b, :n], want[b], True, (name, 'xytp', b))
        if tail is not None:
            assert (got[b, n:].view(np.uint32) == tail).all(), (name, 'xytp rows behind counts[b] were written', b)


def _assert_ordered(c, name, out, lossfn):
    """The ordered batch `out` against the oracle: check_ordered, and the offsets table of FocusLoss.order_events on the oracle's
    time-ordered tensor."""
    ev, num_pos, _ = IC.expected(name)
    assert out['num_pos_events'] == num_pos and 'event_offsets' in out
    got, offs = out['events'].cpu().numpy(), out['event_offsets'].cpu().numpy()
    assert got.shape == ev.shape
    IC.check_ordered(got, offs, num_pos, ev, c.nb, c.sp, c.hq)
    unordered = {'events': torch.tensor(ev, device=DEV), 'num_pos_events': num_pos}          # (a copy: the oracle's array is read-only)
    two = lossfn.order_events(unordered)
    assert torch.equal(out['event_offsets'], two['event_offsets'])
    IC.check_ordered(two['events'].cpu().numpy(), offs, num_pos, ev, c.nb, c.sp, c.hq)
    if name in IC.MULTI_STRIP_CASES:
        assert (offs.shape[2] - 1) // c.nb > 1          # the borders between LUT strips exist on this image
    return unordered


# ---- the public API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_ingest_case_equals_the_oracle(name):
    """events, num_pos_events and xytp[b, :n] of every sample, plain route."""
    c = IC.cases()[name]
    ev, num_pos, _ = IC.expected(name)
    out = _ingest(c, voxel=True)
    assert out['num_pos_events'] == num_pos and 'event_offsets' not in out
    assert tuple(out['events'].shape) == ev.shape
    _assert_bits(out['events'].cpu().numpy(), ev, c.nan, (name, 'events'))
    _assert_xytp(c, out['xytp'], name)


@pytest.mark.parametrize('name', IC.ORDERED_CASES)
def test_ingest_case_ordered_route(name):
    """order_for=: the bucket layout stated by check_ordered, the offsets of order_events, xytp as on the plain route; on the
    strips and degenerate-time cases the loss, its gradient and the IWEs equal those of the time-ordered batch.  The batch with
    M == 0 gives [B, 0, 6] on both routes."""
    from oracle import focus_oracle as O
    c = IC.cases()[name]
    L = _loss_of(c)
    out = _ingest(c, ordered=True, voxel=True)
    ev, num_pos, _ = IC.expected(name)
    assert tuple(out['events'].shape) == ev.shape
    unordered = _assert_ordered(c, name, out, L)
    _assert_xytp(c, out['xytp'], name)
    if name == 'all_dropped':
        assert tuple(out['events'].shape) == (c.B, 0, 6) == tuple(_ingest(c)['events'].shape)
        assert not out['event_offsets'].any()
    else:
        assert (ev[:, :num_pos, 5] == 1).any() and (ev[:, num_pos:, 5] == 1).any()          # both polarity blocks are populated
    if not (name.startswith('strips') or name == 'degenerate_time'):
        return
    g = torch.Generator().manual_seed(1)
    times = torch.cat((torch.tensor([0.41]), O.bin_mid_times(c.nb)))
    traj = O.trajectories_at(torch.randn(c.B, 1, 2, c.H, c.W, generator=g), times, O.tile_mask((c.H, c.W), 4), 1, 'polynomial')
    res = []
    for batch in (unordered, {k: out[k] for k in ('events', 'num_pos_events', 'event_offsets')}):
        tg = traj.to(DEV).requires_grad_(True)
        loss, _, misc = L.calc(tg, times.to(DEV), batch)
        loss.backward()
        res.append((loss.detach(), tg.grad, misc['iwes']))
    assert bool(torch.isfinite(res[0][0])) and bool(res[0][1].any())
    for a, b, what in zip(res[0], res[1], ('loss', 'gradient', 'iwes')):
        assert torch.equal(a, b), (name, what)


# ---- the raw ABI into dirty memory ------------------------------------------------------------------------------------------
NAN_BITS = 0x7FC00000 | 0x1234          # a NaN no arithmetic produces


@pytest.mark.parametrize('ordered', [False, True], ids=['plain', 'ordered'])
@pytest.mark.parametrize('name', IC.RAW_ABI_CASES)
def test_raw_abi_into_dirty_memory(name, ordered):
    """The calls of utils/ingest.py in their order, with `events` and `xytp` pre-filled with NaN, `offsets` and the batch maxima
    with -1 and both workspaces with 0xFF bytes: the outputs equal the oracle, so no row -- padding included -- keeps what was
    there, and no kernel relies on memory it was not handed zeroed."""
    from motionpriorcmax_amd import _lib as C
    from motionpriorcmax_amd.ops import _call, _lut_strips, _ptr, _query, make_shape
    c = IC.cases()[name]
    dev = torch.device(DEV)
    (x, y, t, p), counts = _inputs(c)
    cnt = torch.from_numpy(counts).to(dev)
    ev, num_pos, _ = IC.expected(name)
    dirty = lambda n: torch.full((max(n, 256),), 0xFF, dtype=torch.uint8, device=dev)          # noqa: E731
    nans = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)          # noqa: E731
    shape = C.IngestShape(B=c.B, N=c.N, H=c.H, W=c.W, nb=c.nb)
    ws = dirty(_query('mpc_ingest_workspace_bytes', dev, ctypes.byref(shape)))
    out_max = torch.full((2,), -1, dtype=torch.int32, device=dev)
    _call('mpc_ingest_count', dev, ctypes.byref(shape), _ptr(x), _ptr(y), _ptr(t), _ptr(p), _ptr(cnt), _ptr(out_max), _ptr(ws))
    max_pos, max_neg = (int(v) for v in out_max.tolist())
    assert (max_pos, max_neg) == (num_pos, ev.shape[1] - num_pos)
    events, xytp = nans(c.B, max_pos + max_neg, 6), nans(c.B, c.N, 4)
    if not ordered:
        _call('mpc_ingest_scatter', dev, ctypes.byref(shape), _ptr(x), _ptr(y), _ptr(t), _ptr(p), _ptr(cnt), max_pos, max_neg,
              _ptr(events), _ptr(xytp), _ptr(ws))
        _assert_bits(events.cpu().numpy(), ev, c.nan, (name, 'events'))
    else:
        L = _loss_of(c)
        lshape = make_shape(L._cfg, c.B, max_pos + max_neg, max_pos, 1)
        ncs = _lut_strips(lshape, dev)
        assert ncs > 0
        ws2 = dirty(_query('mpc_ingest_ordered_workspace_bytes', dev, ctypes.byref(shape), ctypes.byref(lshape)))
        offs = torch.full((c.B, 2, c.nb * ncs + 1), -1, dtype=torch.int32, device=dev)
        _call('mpc_ingest_scatter_ordered', dev, ctypes.byref(shape), ctypes.byref(lshape), _ptr(x), _ptr(y), _ptr(t), _ptr(p),
              _ptr(cnt), max_pos, max_neg, _ptr(events), _ptr(offs), _ptr(xytp), _ptr(ws), _ptr(ws2))
        _assert_ordered(c, name, {'events': events, 'num_pos_events': max_pos, 'event_offsets': offs}, L)
    _assert_xytp(c, xytp, name, tail=NAN_BITS)


# ---- the rectification-map source -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('voxel', [False, True], ids=['events', 'events+xytp'])
@pytest.mark.parametrize('ordered', [False, True], ids=['plain', 'ordered'])
def test_map_route_equals_the_float_route_on_gathered_coordinates(ordered, voxel):
    """Raw indices + map against the float entry points fed the gathered coordinates ((-2, -2) for an index outside the map),
    bit for bit; the oracle on the gathered coordinates is what test_ingest_case_equals_the_oracle holds both to."""
    c = IC.cases()['map']
    ev, num_pos, _ = IC.expected('map')
    got = _ingest(c, ordered=ordered, voxel=voxel)
    ref = _ingest(c, ordered=ordered, voxel=voxel, gathered=True)
    assert got['num_pos_events'] == ref['num_pos_events'] == num_pos
    assert (got['xytp'] is None) == (ref['xytp'] is None) == (not voxel)
    if voxel:
        _assert_xytp(c, got['xytp'], 'map')
        _assert_xytp(c, ref['xytp'], 'map')
    if not ordered:
        assert torch.equal(got['events'].view(torch.int32), ref['events'].view(torch.int32))
        _assert_bits(got['events'].cpu().numpy(), ev, c.nan, ('map', 'events'))
        return
    assert torch.equal(got['event_offsets'], ref['event_offsets'])
    _assert_ordered(c, 'map', got, _loss_of(c))
    _assert_ordered(c, 'map', ref, _loss_of(c))
