"""The bucket key of an event -- (time bin, LUT strip) of its own LUT cell, csrc/ev_key_device.h -- on its four routes over the same
rows: the forward's backward records (k_ev_bin) with their exact-size buckets (k_ev_count / k_ev_prefix), the ordering sort
(ops.event_bucket_order: k_evo_*), ingest straight into the ordered layout (k_ingest_keycount / k_ingest_scatter_ordered) and the
ordered backward (k_lut_accum over the offsets table).  A route that filed one row under another key would show as a wrong table
(a, b) or as a gradient that differs between the record and the ordered backward (c): integer sums, so every comparison is exact.

The rows sit where the key changes: for every cell row r in 0 .. hq an event at y = r * sp and one at the float below it, y < 0
and y >= H, bin columns -1 and nb, both polarities, padding rows inside and at the end of the blocks, M no multiple of 256 and
more than one chunk of the sort per block.  sp = 4 takes the reciprocal branch of mpc_div_sp, sp = 3 the division.

MPC_EV_CSTRIP_KB=1 (strips of 4 cell rows: 5 and 7 strips) and MPC_EV_EXACT_ABOVE_MB=0 (exact-size buckets) are read once per
process, so the cases run in one child interpreter, as those of test_gpu_event_cases.py do."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV = {'MPC_EV_CSTRIP_KB': '1', 'MPC_EV_EXACT_ABOVE_MB': '0'}
#        B, nb, H,  W,  sp, rows per strip, strips
CASES = {'first': (2, 3, 80, 64, 4, 4, 5),
         'second': (2, 3, 80, 48, 3, 4, 7)}          # hq = 27: the last strip has 3 rows; the v / sp branch of mpc_div_sp
REPS = 12                                            # copies of the edge rows (other columns, times): > 2048 rows per block


def _dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _loss(H, W, nb, sp):
    from motionpriorcmax_amd import LossFactory
    cfg = dict(image_shape=(H, W), num_tref=1, num_bins=nb, num_knn=8, smooth_weight=0.003, lut_superpixel_size=sp,
               focus_loss_norm='l1', dist_norm='l2', scale_iwe_by_dt=True, mask_image_border=True, polarity_aware_batching=True,
               interpolation_scheme='mean', smooth_type='on_flow_to_tref')
    return LossFactory.get_loss_calculator('FOCUS', cfg)


def _edge_ys(H, sp, hq):
    r = np.arange(hq + 1, dtype=np.float32) * np.float32(sp)
    return np.concatenate((r, np.nextafter(r, np.float32(-np.inf)), np.float32([-5.5, -0.25, H, H + 3.25])))


def _rows(name):
    """events [B, M, 6] (y, x, t, p, bin, valid), num_pos: every edge height with every bin column value -1 .. nb in both
    polarity blocks, REPS times; 5 % of the rows zeroed inside the blocks, a few padding rows at the end of each."""
    B, nb, H, W, sp, _, _ = CASES[name]
    hq = -(-H // sp)
    rng = np.random.default_rng(11 if name == 'first' else 12)
    ys = _edge_ys(H, sp, hq)
    y, bn = (a.reshape(-1) for a in np.meshgrid(ys, np.arange(-1, nb + 1, dtype=np.float32), indexing='ij'))
    y, bn = np.tile(y, REPS), np.tile(bn, REPS)
    npos, nneg = len(y) + 37, len(y) + 12                      # + padding rows at the end of the block
    M = npos + nneg
    assert M % 256 != 0 and len(y) > 2048
    ev = np.zeros((B, M, 6), dtype=np.float32)
    for b in range(B):
        for pol, r0 in ((1.0, 0), (0.0, npos)):
            p = rng.permutation(len(y))
            blk = ev[b, r0:r0 + len(y)]
            blk[:, 0], blk[:, 4] = y[p], bn[p]
            blk[:, 1] = rng.uniform(0, W, len(y)).astype(np.float32)
            blk[:, 2] = rng.uniform(0, 1, len(y)).astype(np.float32)
            blk[:, 3], blk[:, 5] = pol, 1.0
            blk[rng.random(len(y)) < 0.05] = 0.0
    return ev, npos


def _keys(rows, nb, sp, hq, ncs):
    """The key definition in numpy: clamped bin * NCS + clamped cell row // CSR, CSR = ceil(hq / NCS); nb * NCS for a padding row."""
    csr = -(-hq // ncs)
    it = np.clip(rows[:, 4].astype(np.int64), 0, nb - 1)
    q = rows[:, 0] * (np.float32(1) / np.float32(sp)) if sp & (sp - 1) == 0 else rows[:, 0] / np.float32(sp)
    iy = np.clip(np.floor(q).astype(np.int64), 0, hq - 1)
    return np.where(rows[:, 5] == 0, nb * ncs, it * ncs + iy // csr)


def _check_table(ev_in, ev_out, offs, num_pos, nb, sp, hq, ncs):
    """offs equals the table counted from the key definition over the rows of ev_in, and every row of ev_out lies in the bucket its
    key names (so the multiset of rows of every bucket is that of ev_in's rows with that key)."""
    B, M, _ = ev_in.shape
    nk = nb * ncs
    assert offs.shape == (B, 2, nk + 1)
    for b in range(B):
        for pol, (r0, r1) in enumerate(((0, num_pos), (num_pos, M))):
            k_in = _keys(ev_in[b, r0:r1], nb, sp, hq, ncs)
            want = r0 + np.concatenate(([0], np.cumsum(np.bincount(k_in, minlength=nk + 1))[:nk]))
            np.testing.assert_array_equal(offs[b, pol], want, err_msg=f'sample {b} block {pol}')
            k_out = _keys(ev_out[b, r0:r1], nb, sp, hq, ncs)
            np.testing.assert_array_equal(k_out, np.sort(k_in), err_msg=f'a row outside its bucket: sample {b} block {pol}')
            o_in, o_out = np.argsort(k_in, kind='stable'), np.arange(r1 - r0)
            for k in np.unique(k_in):
                assert sorted(map(bytes, ev_in[b, r0:r1][o_in[np.sort(k_in) == k]])) == sorted(map(bytes, ev_out[b, r0:r1][o_out[k_out == k]])), (b, pol, k)


def _raw_window(ev, num_pos, H, W, rng):
    """The rows of `ev` as a raw (x, y, t_us, p) window in time order, both polarities mixed; padding rows left out (ingest drops
    the rows outside the image itself, and takes the bins from the times)."""
    B = ev.shape[0]
    per = []
    for b in range(B):
        keep = ev[b, :, 5] != 0
        x, y, p = ev[b, keep, 1], ev[b, keep, 0], ev[b, keep, 3]
        o = rng.permutation(len(x))
        per.append((x[o], y[o], np.sort(rng.integers(10**6, 2 * 10**6, len(x))).astype(np.int64), p[o]))
    N = max(len(a[0]) for a in per) + 3                       # (rows behind counts[b] are never read)
    out = [np.zeros((B, N), dtype=np.int64 if i == 2 else np.float32) for i in range(4)]
    for b, a in enumerate(per):
        for dst, src in zip(out, a):
            dst[b, :len(src)] = src
    return out, np.array([len(a[0]) for a in per], dtype=np.int32)


def _run_case(name):
    from motionpriorcmax_amd import _lib as C, ops
    from motionpriorcmax_amd.utils import ingest_events
    B, nb, H, W, sp, csr_want, ncs_want = CASES[name]
    hq = -(-H // sp)
    L = _loss(H, W, nb, sp)
    cfg, dev = L._cfg, _dev()
    ev, num_pos = _rows(name)
    M = ev.shape[1]
    shape = ops.make_shape(cfg, B, M, num_pos, 0, K=0)
    ncs = ops._lut_strips(shape, dev)
    print(f'{name}: M {M} hq {hq} strips {ncs} rows per strip {-(-hq // ncs)}')
    assert ncs >= 5 and (ncs, -(-hq // ncs)) == (ncs_want, csr_want), (ncs, hq)
    assert {int(k) for k in np.unique(_keys(ev[0], nb, sp, hq, ncs))} == set(range(nb * ncs + 1))          # every bucket is populated

    # (a) the ordering sort against the key definition
    evd = torch.from_numpy(ev).to(dev)
    evo, offs = ops.event_bucket_order(cfg, evd, num_pos)
    _check_table(ev, evo.cpu().numpy(), offs.cpu().numpy(), num_pos, nb, sp, hq, ncs)

    # (b) ingest into the ordered layout against the ordering sort of the plain ingest's tensor
    (x, y, t, p), counts = _raw_window(ev, num_pos, H, W, np.random.default_rng(5))
    args = [torch.from_numpy(a).to(dev) for a in (x, y, t, p)]
    plain = ingest_events(*args, torch.from_numpy(counts), (H, W), nb)
    with ops.KernelTimer() as kt:
        ordered = ingest_events(*args, torch.from_numpy(counts), (H, W), nb, order_for=L)
    assert {'k_ingest_keycount', 'k_ingest_scatter_ordered'} <= set(kt.summary()), set(kt.summary())
    pe, pn = plain['events'], plain['num_pos_events']
    assert ordered['num_pos_events'] == pn and 0 < pn < pe.shape[1]
    two, offs2 = ops.event_bucket_order(cfg, pe, pn)
    assert torch.equal(ordered['event_offsets'], offs2)
    ncs_i = ops._lut_strips(ops.make_shape(cfg, B, pe.shape[1], pn, 0, K=0), dev)
    assert ncs_i == ncs
    _check_table(pe.cpu().numpy(), ordered['events'].cpu().numpy(), offs2.cpu().numpy(), pn, nb, sp, hq, ncs)
    _check_table(pe.cpu().numpy(), two.cpu().numpy(), offs2.cpu().numpy(), pn, nb, sp, hq, ncs)

    # (c) record backward (exact-size buckets) against ordered backward: the same LUT and adjoint image
    rng = np.random.default_rng(3)
    lut = torch.from_numpy((2.0 * rng.standard_normal((B, nb, hq, -(-W // sp), 1, 2))).astype(np.float32)).to(dev)
    gimg = torch.from_numpy(rng.standard_normal((B, 2, H, W)).astype(np.float32)).to(dev)
    t_ref = torch.tensor([0.4], device=dev)
    scal = torch.ones(C.SCAL_COUNT, device=dev)
    gout = torch.tensor([1.0], device=dev)
    grads = []
    with ops.KernelTimer() as kt:
        for rows, table in ((evd, None), (evo, offs)):
            ws = ops.alloc_workspace(shape, dev)
            ops.event_splat_fwd(shape, rows, lut, t_ref, ws)
            grads.append(ops.event_splat_bwd(shape, rows, lut, t_ref, gimg, scal, gout, torch.empty_like(lut), None, ws, table))
    assert {'k_ev_bin', 'k_ev_count', 'k_ev_prefix', 'k_lut_accum'} <= set(kt.summary()), set(kt.summary())
    assert grads[0].abs().max() > 0
    assert torch.equal(grads[0], grads[1]), (grads[0] - grads[1]).abs().max().item()


@functools.lru_cache(maxsize=None)
def _child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, '-m', 'pytest', 'tests/test_gpu_event_keys.py', '-q', '-s', '-rA', '-m', 'gpu'],
                          cwd=root, env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize('name', list(CASES))
def test_four_routes_file_the_rows_alike(name):
    if all(os.environ.get(k) == v for k, v in ENV.items()):
        return _run_case(name)
    r = _child()          # one child interpreter for all the cases
    print('\n'.join(line for line in r.stdout.splitlines() if f'{name}: M ' in line), flush=True)
    assert f'PASSED tests/test_gpu_event_keys.py::test_four_routes_file_the_rows_alike[{name}]' in r.stdout and 'skipped' not in r.stdout, \
        (r.stdout[-2500:], r.stderr[-500:])
