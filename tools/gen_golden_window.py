#!/usr/bin/env python3
"""Fixtures g14_window_<case>.npz for utils.ingest_raw_events: the loss events of the EVIMO2 and MultiFlow configurations as the
UNMODIFIED reference builds them from a raw window --
  EVIMO2     EVIMO2_Datasubset(..., provide_raw_events=True)[i] (src/loader/evimo2/datasubset.py:135-229) on a synthetic dataset
             directory, then sequence_collate_fn (src/modules/data_loading.py:59-84) on three samples, in both polarity modes;
  MultiFlow  Sample(...).get_events_context() (src/loader/multiflow/sample.py:224-236), the split of
             src/loader/multiflow/datasubset.py:149-156 and the same collate.

    python tools/gen_golden_window.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_cvx.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own
files are imported as they are, and only DATA is written.  Two stand-ins are installed HERE, in this process only: a dict-backed
`h5py.File` (the stub under oracle/ is an empty class) and `pytorch_lightning.LightningDataModule = object` (the base class of
data_loading.DataModule, which is not used).  Deterministic: a second run reproduces the files bit for bit.

The EVIMO2 inputs are chosen so that the fixture tells the reference's float32 arithmetic from a float64 one: absolute time
starts at 100 s (one fp32 ulp of a microsecond stamp is 8 us there), and the tool asserts that in every sample at least one
event's bin, or the number of kept events, differs from a float64 evaluation of the same formulas.

Every file holds the padded window x, y [B, N], t_us [B, N] int64, p [B, N], counts [B], num_bins, and the reference's collated
`events` [B, M, 6] with `num_pos_events`; EVIMO2 files also flow_duration_ms, x_scale, y_scale and n_differs [B] (events per
sample whose bin differs from the float64 evaluation) and kept64 [B]; the MultiFlow file holds both collates
(events_single: without the polarity split)."""
import argparse
import os
import sys
import tempfile

import numpy as np

NUM_BINS = 41
FLOW_TIME_MS = 300
T0_S = 100.0


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


class FakeH5File:
    """Dict-backed stand-in for h5py.File: FILES[path] = {name: array}; read-only, usable as a context manager."""
    FILES = {}

    def __init__(self, path, mode='r'):
        self._d = self.FILES[os.path.abspath(str(path))]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, key):
        return self._d[key]


def pad(rows, dtype):
    n = max(len(r) for r in rows)
    out = np.zeros((len(rows), n), dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'oracle', 'stubs'))
    sys.path.insert(1, args.ref)
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

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)

    # ---- EVIMO2: 1.3 s of events from 100 s on, three flow stamps 0.1 s apart -> windows of 0.4 s + 0.3 s
    g = np.random.default_rng(1400)
    n_ev = 7600
    t_s = T0_S + np.sort(g.integers(0, 1_300_000, n_ev)).astype(np.float64) / 1e6          # seconds, as the dataset stores them
    xy = np.stack((g.integers(0, 640, n_ev), g.integers(0, 480, n_ev)), axis=1).astype(np.int16)
    pol = (g.random(n_ev) > 0.45).astype(np.uint8)
    flow_time = T0_S + np.array([0.5, 0.6, 0.7]) + g.integers(0, 1000, 3) / 1e6
    with tempfile.TemporaryDirectory(prefix='g14_') as td:
        np.save(os.path.join(td, 'dataset_events_xy.npy'), xy)
        np.save(os.path.join(td, 'dataset_events_p.npy'), pol)
        np.save(os.path.join(td, 'dataset_events_t.npy'), t_s)
        k = len(flow_time)
        FakeH5File.FILES[os.path.abspath(os.path.join(td, 'dataset_multiflow_10steps_vis.h5'))] = {
            'time': flow_time, 'multiflow': np.zeros((k, 10, 2, 480, 640), np.float32), 'obj_id_mask': np.zeros((k, 480, 640), np.float32)}
        for split in (True, False):
            ds = EVIMO2_Datasubset(Path(td), False, NUM_BINS, 50, flow_time=FLOW_TIME_MS, provide_raw_events=True,
                                   polarity_aware_batching=split)
            assert len(ds) == k and ds.start_index == 0
            batch = sequence_collate_fn([ds[i] for i in range(k)])
            # the raw window of sample i, by the expressions of datasubset.py:143-154
            xs, ys, ts, ps = [], [], [], []
            for i in range(k):
                a, b = int(ds.prev2evt[i]), int(ds.next2evt[i])
                xs.append(xy[a:b, 0].astype('int32')); ys.append(xy[a:b, 1].astype('int32'))
                ts.append(np.array(t_s[a:b] * 1e6).astype('int'))
                ps.append(1 - pol[a:b].astype('int'))
            events = batch[DataLoading.EVENTS].numpy()
            assert events.dtype == np.float32
            # the same formulas in float64: the fixture must tell the two apart in every sample
            n_differs, kept64 = [], []
            valid = events[..., 5] == 1
            for i in range(k):
                t = ts[i].astype(np.float64)
                start = t[-1] - FLOW_TIME_MS * 1e3
                keep = t > start
                tn = (t[keep] - start) / (t[-1] - start)
                bins = np.searchsorted(np.linspace(0, 1, NUM_BINS + 1), tn) - 1
                bins[bins == -1] = 0
                kept32 = int(valid[i].sum())
                pk = ps[i][len(ps[i]) - kept32:]          # the kept events are a suffix of the window
                order = np.concatenate((np.nonzero(pk == 1)[0], np.nonzero(pk == 0)[0])) if split else np.arange(kept32)
                ref_bins = np.empty(kept32, np.float32)
                ref_bins[order] = events[i][valid[i]][:, 4]          # the reference's bins, back in input order
                kept64.append(int(keep.sum()))
                m = min(kept32, kept64[-1])
                n_differs.append(int((ref_bins[kept32 - m:] != bins[len(bins) - m:]).sum()))
                assert n_differs[-1] != 0 or kept64[-1] != int(valid[i].sum()), f'sample {i}: float64 gives the same result'
            name = 'g14_window_evimo2_' + ('split' if split else 'single')
            path = os.path.join(args.out, name + '.npz')
            save_npz(path, dict(x=pad(xs, np.int32), y=pad(ys, np.int32), t_us=pad(ts, np.int64), p=pad(ps, np.int64),
                                counts=np.array([len(a) for a in ts], np.int32), num_bins=np.int64(NUM_BINS),
                                flow_duration_ms=np.int64(FLOW_TIME_MS), events=events,
                                num_pos_events=np.int64(batch[DataLoading.NUM_POS_EVENTS]),
                                x_scale=np.float64(batch[DataLoading.X_SCALE]), y_scale=np.float64(batch[DataLoading.Y_SCALE]),
                                n_differs=np.array(n_differs, np.int64), kept64=np.array(kept64, np.int64),
                                kept=valid.sum(1).astype(np.int64)))
            print(f'{name}: {os.path.getsize(path)} B  windows {[len(a) for a in ts]}  kept {valid.sum(1).tolist()} (float64: {kept64})  '
                  f'bins that differ from float64 {n_differs}')

    # ---- MultiFlow: three sample directories, events over the whole second, context window 0.4 s .. 0.9 s
    samples = []
    with tempfile.TemporaryDirectory(prefix='g14_') as td:
        for i in range(3):
            sd = os.path.join(td, f'seq{i}')
            for sub in ('images', 'flow', 'events'):
                os.makedirs(os.path.join(sd, sub))
            for f in ('images/0400000.png', 'images/0900000.png', 'flow/0500000.h5', 'events/events.h5'):
                open(os.path.join(sd, f), 'wb').close()          # placeholders: only their existence and names are read
            g = np.random.default_rng(1410 + i)
            n = 7000 + 900 * i
            FakeH5File.FILES[os.path.abspath(os.path.join(sd, 'events', 'events.h5'))] = {
                't': np.sort(g.integers(0, 1_000_000, n)).astype(np.int64), 'x': g.integers(0, 512, n).astype(np.uint16),
                'y': g.integers(0, 384, n).astype(np.uint16), 'p': (g.random(n) > 0.55).astype(np.uint8)}
            s = Sample(Path(sd), 384, 512, NUM_BINS, load_voxel_grid=False)
            raw = s._get_events(s.flow_ref_ts_us, s.flow_ref_ts_us + s.prediction_time_us)          # the window get_events_context cuts
            samples.append((raw, s.get_events_context()))
        out = {}
        for split in (True, False):
            items = []
            for raw, ev in samples:          # multiflow/datasubset.py:149-156
                items.append({DataLoading.POS_EVENTS: ev[ev[:, 3] == 1], DataLoading.NEG_EVENTS: ev[ev[:, 3] == 0]} if split
                             else {DataLoading.EVENTS: ev})
            batch = sequence_collate_fn(items)
            out['events' if split else 'events_single'] = batch[DataLoading.EVENTS].numpy()
            out['num_pos_events' if split else 'num_pos_events_single'] = np.int64(batch[DataLoading.NUM_POS_EVENTS])
        raws = [r for r, _ in samples]
        out.update(x=pad([r['x'] for r in raws], np.int32), y=pad([r['y'] for r in raws], np.int32),
                   t_us=pad([r['t'] for r in raws], np.int64), p=pad([r['p'] for r in raws], np.int64),
                   counts=np.array([len(r['t']) for r in raws], np.int32), num_bins=np.int64(NUM_BINS))
        assert out['events'].dtype == np.float32
        path = os.path.join(args.out, 'g14_window_multiflow.npz')
        save_npz(path, out)
        print(f"g14_window_multiflow: {os.path.getsize(path)} B  windows {out['counts'].tolist()}  num_pos_events {int(out['num_pos_events'])}")


if __name__ == '__main__':
    main()
