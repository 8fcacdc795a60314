#!/usr/bin/env python3
"""Fixtures g17_targets_<case>.npz for utils.flow_targets: the ground-truth flow targets of the EVIMO2 and MultiFlow configurations
as the UNMODIFIED reference prepares them from the raw multi-step flow --
  EVIMO2     EVIMO2_Datasubset(...)[i] (src/loader/evimo2/datasubset.py:135-204: FLOW, FLOW_VALID, ID_MASK) on a synthetic dataset
             directory, then sequence_collate_fn (src/modules/data_loading.py:59-84);
  MultiFlow  Sample(..., downsample=True).get_flow_gt(100) (src/loader/multiflow/sample.py:108-139) on synthetic sample directories.

    python tools/gen_golden_targets.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_window.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files
are imported as they are, only DATA is written, and the same two stand-ins are installed in this process only (a dict-backed
`h5py.File`, `pytorch_lightning.LightningDataModule = object`).  Deterministic: a second run reproduces the files bit for bit.

EVIMO2_Datasubset takes its sizes from four instance attributes (original_height / original_width / resize_height / resize_width);
they are set on the constructed object, which leaves the reference as it is, and the events the dataset also reads lie inside the
small image.

Every file holds the raw inputs (EVIMO2: raw_flow [B, S, 2, H, W] with NaN, obj_id_mask [B, H, W]; MultiFlow: raw_flow [B, S, H, W, 2]),
the reference's flow (and flow_valid, id_mask, x_scale, y_scale), flow64 -- the same formulas in float64 on the fp32 inputs with the
fp32 source indices and weights (tests/flow_targets_oracle.py) -- and err_ref = max|flow - flow64|.  The tool asserts err_ref > 0
(case d, same size: every weight is 0 or 1 and the blend is exact, so there err_ref == 0 is asserted instead and the rule
max|out - flow64| <= 2 err_ref asks for equality) and that the valid share of every EVIMO2 case lies strictly between 0 and 1.
The MultiFlow file holds two shapes: raw_flow / flow / flow64 / err_ref and the same names with the suffix _odd.

  a  EVIMO2 20x28 -> 16x24, B=2, S=6   the shipped 1.25 ratio; NaN blobs, single-channel NaNs, one all-NaN step, one without NaN; ids to 255
  b  EVIMO2 21x27 -> 13x32, B=1, S=2   down in y, up in x, odd sizes; nearest tap != bilinear i0
  c  EVIMO2 10x12 -> 7x5,   B=3, S=1   Wo not a multiple of 4
  d  EVIMO2 9x11  -> 9x11,  B=1, S=1   same size: flow bit-equal to the zeroed input
  e  MultiFlow 20x28 -> 10x14 and 21x27 -> 10x13, B=2, S=3"""
import argparse
import os
import sys
import tempfile

import numpy as np

from gen_golden_window import FakeH5File, save_npz

NUM_BINS = 41
T0_S = 100.0
EVIMO2_CASES = {'a': (20, 28, 16, 24, 2, 6), 'b': (21, 27, 13, 32, 1, 2), 'c': (10, 12, 7, 5, 3, 1), 'd': (9, 11, 9, 11, 1, 1)}


def synth_flow(g, B, S, H, W, case):
    """A smooth field plus noise, a few px in size, with the NaN pattern the case is for."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    raw = np.empty((B, 10, 2, H, W), np.float32)          # the file holds ten steps; the loader takes the first S
    for b in range(B):
        for s in range(10):
            a, c = g.uniform(-0.4, 0.4, 2), g.uniform(-6, 6, 2)
            raw[b, s, 0] = c[0] + a[0] * (xx - W / 2) + 1.5 * np.sin(yy / 3.1 + s) + g.normal(0, 0.7, (H, W))
            raw[b, s, 1] = c[1] + a[1] * (yy - H / 2) + 1.5 * np.cos(xx / 2.7 - s) + g.normal(0, 0.7, (H, W))
    for b in range(B):
        for s in range(S):
            if case == 'a' and (b, s) == (0, 4):
                continue                                            # one step without NaN
            if case == 'a' and (b, s) == (1, 2):
                raw[b, s] = np.nan                                  # one all-NaN step
                continue
            for _ in range(2):                                      # blobs: both channels
                y, x, h, w = g.integers(0, H - 2), g.integers(0, W - 2), g.integers(2, max(3, H // 3)), g.integers(2, max(3, W // 3))
                raw[b, s, :, y:y + h, x:x + w] = np.nan
            single = g.random((2, H, W)) < 0.06                    # one channel alone
            single[1] &= ~single[0]
            raw[b, s][single] = np.nan
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'oracle', 'stubs'))
    sys.path.insert(1, args.ref)
    sys.path.insert(2, os.path.join(root, 'tests'))
    import torch
    import h5py
    import pytorch_lightning
    h5py.File = FakeH5File
    pytorch_lightning.LightningDataModule = object
    from pathlib import Path
    from src.loader.evimo2.datasubset import EVIMO2_Datasubset          # reference, unmodified
    from src.loader.multiflow.sample import Sample                      # reference, unmodified
    from src.loader.utils.keys import DataLoading                       # reference, unmodified
    from src.modules.data_loading import sequence_collate_fn            # reference, unmodified
    import flow_targets_oracle as O                                     # own restatement (float64 yardstick)

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)

    for n, (case, (H, W, Ho, Wo, B, S)) in enumerate(EVIMO2_CASES.items()):
        g = np.random.default_rng(1700 + n)
        n_ev = 900
        t_s = T0_S + np.sort(g.integers(0, 1_300_000, n_ev)).astype(np.float64) / 1e6
        xy = np.stack((g.integers(0, W, n_ev), g.integers(0, H, n_ev)), axis=1).astype(np.int16)          # inside the small image
        pol = (g.random(n_ev) > 0.45).astype(np.uint8)
        flow_time = T0_S + 0.5 + 0.1 * np.arange(B) + g.integers(0, 1000, B) / 1e6
        raw10 = synth_flow(g, B, S, H, W, case)
        ids = g.integers(0, 256, (B, H, W)).astype(np.uint8)
        ids[:, 0, 0] = 255
        with tempfile.TemporaryDirectory(prefix='g17_') as td:
            np.save(os.path.join(td, 'dataset_events_xy.npy'), xy)
            np.save(os.path.join(td, 'dataset_events_p.npy'), pol)
            np.save(os.path.join(td, 'dataset_events_t.npy'), t_s)
            FakeH5File.FILES[os.path.abspath(os.path.join(td, 'dataset_multiflow_10steps_vis.h5'))] = {
                'time': flow_time, 'multiflow': raw10.copy(), 'obj_id_mask': ids.copy()}
            ds = EVIMO2_Datasubset(Path(td), False, NUM_BINS, 50, flow_time=50 * S)
            ds.original_height, ds.original_width, ds.resize_height, ds.resize_width = H, W, Ho, Wo
            assert len(ds) == B and ds.start_index == 0
            items = [ds[i] for i in range(B)]
            batch = sequence_collate_fn(items)
        raw = raw10[:, :S]
        flow = batch[DataLoading.FLOW].numpy()
        valid = batch[DataLoading.FLOW_VALID].numpy()
        idm = batch[DataLoading.ID_MASK].numpy().reshape(B, Ho, Wo)          # (one sample: the collate stacks the squeezed [Ho, Wo])
        assert flow.dtype == np.float32 and flow.shape == (B, S, 2, Ho, Wo) and valid.dtype == np.bool_ and valid.shape == (B, S, Ho, Wo)
        assert idm.dtype == np.float32 and idm.max() == 255
        assert np.isfinite(flow).all()
        flow64, valid64, ids64, xs, ys = O.evimo2(raw, (Ho, Wo), ids, dtype=np.float64)
        assert np.array_equal(valid64, valid) and np.array_equal(ids64, idm), case
        err_ref = float(np.abs(flow.astype(np.float64) - flow64).max())
        share = float(valid.mean())
        assert 0.0 < share < 1.0, (case, share)
        assert (err_ref == 0.0) if case == 'd' else (err_ref > 0.0), (case, err_ref)
        if case == 'd':
            assert np.array_equal(flow, np.where(np.isnan(raw), np.float32(0), raw))
        if case == 'a':
            assert not valid[1, 2].any() and not np.isnan(raw[0, 4]).any()
            assert (np.isnan(raw[:, :, 0]) ^ np.isnan(raw[:, :, 1])).any()
        x_scale, y_scale = ds.resize_width / W, ds.resize_height / H          # datasubset.py:185-186 (returned only with raw events)
        assert (xs, ys) == (x_scale, y_scale)
        path = os.path.join(args.out, f'g17_targets_{case}.npz')
        save_npz(path, dict(raw_flow=raw, obj_id_mask=ids, out_size=np.array([Ho, Wo], np.int64), flow=flow, flow_valid=valid, id_mask=idm,
                            x_scale=np.float64(x_scale), y_scale=np.float64(y_scale), flow64=flow64, err_ref=np.float64(err_ref)))
        print(f'g17_targets_{case}: {os.path.getsize(path)} B  {H}x{W} -> {Ho}x{Wo}  B={B} S={S}  valid share {share:.3f}  err_ref {err_ref:.3g}')

    # ---- MultiFlow: two sample directories per shape, flow files at 0.5, 0.6, 0.7 s
    out = {}
    for suffix, (H, W) in (('', (20, 28)), ('_odd', (21, 27))):
        g = np.random.default_rng(1710 + H)
        raw = (g.normal(0, 4, (2, 3, H, W, 2)) + g.uniform(-8, 8, (2, 3, 1, 1, 2))).astype(np.float32)
        flows = []
        with tempfile.TemporaryDirectory(prefix='g17_') as td:
            for b in range(2):
                sd = os.path.join(td, f'seq{b}')
                for sub in ('images', 'flow', 'events'):
                    os.makedirs(os.path.join(sd, sub))
                names = ['flow/0500000.h5', 'flow/0600000.h5', 'flow/0700000.h5']
                for f in ['images/0400000.png', 'images/0900000.png', 'events/events.h5'] + names:
                    open(os.path.join(sd, f), 'wb').close()          # placeholders: only their existence and names are read
                for s, f in enumerate(names):
                    FakeH5File.FILES[os.path.abspath(os.path.join(sd, f))] = {'flow': raw[b, s].copy()}
                smp = Sample(Path(sd), H, W, NUM_BINS, load_voxel_grid=False, downsample=True)
                gt = smp.get_flow_gt(100)
                assert gt['timestamps'] == [500000, 600000, 700000]
                flows.append(torch.stack(gt['flow'], dim=0))
        flow = torch.stack(flows, dim=0).numpy()
        assert flow.dtype == np.float32 and flow.shape == (2, 3, 2, H // 2, W // 2)
        flow64 = O.multiflow(raw, dtype=np.float64)
        err_ref = float(np.abs(flow.astype(np.float64) - flow64).max())
        assert err_ref > 0.0
        out.update({'raw_flow' + suffix: raw, 'flow' + suffix: flow, 'flow64' + suffix: flow64, 'err_ref' + suffix: np.float64(err_ref)})
        print(f'g17_targets_e{suffix}: {H}x{W} -> {H // 2}x{W // 2}  err_ref {err_ref:.3g}')
    out.update(x_scale=np.float64(0.5), y_scale=np.float64(0.5))
    path = os.path.join(args.out, 'g17_targets_e.npz')
    save_npz(path, out)
    print(f'g17_targets_e: {os.path.getsize(path)} B')


if __name__ == '__main__':
    main()
