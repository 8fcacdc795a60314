#!/usr/bin/env python3
"""Fixtures g20_dsec_sample.npz and g20_dsec_export.npz for the DSEC rectification inside the ingest, `utils.dsec_flow_targets` /
`dsec_flow_error` and `utils.dsec_flow_png16`, made by the UNMODIFIED reference --
  sample  Sequence.get_data_sample + sequence_collate_fn (src/loader/dsec/loader.py:141-182, 360-415) on synthetic windows: the
          rectification gather, the loss events, the voxel grid, forward_flow / flow_valid from a 16-bit payload;
  export  scale_optical_flow + save_flow (scripts/dsec_inference.py:33-49) on synthetic dense flows.

    python tools/gen_golden_dsec_io.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_targets.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files
are imported as they are and only DATA is written.  There is no dataset on disk: the Sequence is made with object.__new__ and given
the attributes get_data_sample reads, a stand-in `event_slicer` whose get_events hands back the synthetic window, and
`paths_to_forward_flow` pointing at empty temporary files; `imageio.imread` / `imageio.v2.imwrite` (third-party, absent here) are
stand-ins defined below that return the synthetic payload / capture the array save_flow hands over.  The inputs come from
tests/dsec_io_cases.py, which the tests use too.  Deterministic: a second run reproduces the files bit for bit."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

from gen_golden_window import save_npz


class Slicer:
    """event_slicer stand-in: the window of sample `b` as the h5 file holds it (uint16 x / y, uint8 p, int64 t)."""

    def __init__(self, windows):
        self.windows = windows

    def get_events(self, t_start, t_end):
        x, y, t, p = self.windows[int(t_start)]
        assert t.min() >= t_start and t.max() < t_end
        return {'x': x.astype(np.uint16), 'y': y.astype(np.uint16), 't': t.copy(), 'p': p.astype(np.uint8)}


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
    sys.path.insert(3, root)
    import torch
    import imageio                                                      # oracle/stubs: empty
    import pytorch_lightning
    pytorch_lightning.LightningDataModule = object
    payloads, written = {}, []
    imageio.imread = lambda path, format=None: payloads[str(path)].copy()
    v2 = types.ModuleType('imageio.v2')
    v2.imwrite = lambda path, arr, format=None: written.append((str(path), np.array(arr, copy=True)))
    v2.imread = imageio.imread
    imageio.v2 = v2
    sys.modules['imageio.v2'] = v2
    from src.loader.dsec.loader import Sequence, sequence_collate_fn     # reference, unmodified
    from src.loader.dsec.utils import VoxelGrid                          # reference, unmodified
    import dsec_io_cases as K                                            # the cases + own restatements

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)

    # ---- sample: rectification, loss events, voxel grid, flow targets
    m = K.rectify_map()
    x, y, t, p, counts = K.raw_window()
    B = len(counts)
    png = K.payload(B, K.H, K.W)
    seq = object.__new__(Sequence)
    seq.name, seq.phase = 'g20', 'val'
    seq.height, seq.width, seq.num_bins = K.H, K.W, K.NB
    seq.t_bins = np.linspace(0, 1, K.NB + 1)                             # loader.py:62
    seq.polarity_aware_batching = True
    seq.voxel_grid = VoxelGrid((K.NB, K.H, K.W), norm_type='mean_std', quantile=0)          # :65
    seq.rectify_ev_map = m
    t0 = np.array([int(t[b, 0]) for b in range(B)], np.int64)
    seq.timestamps_flow = np.stack((t0, t0 + 100000), axis=1)
    seq.indices = list(range(10, 10 + B))
    seq.event_slicer = Slicer({int(t0[b]): (x[b, :c], y[b, :c], t[b, :c], p[b, :c]) for b, c in enumerate(counts)})
    with tempfile.TemporaryDirectory(prefix='g20_') as td:
        seq.paths_to_forward_flow = []
        for b in range(B):
            f = os.path.join(td, f'{10 + b:06d}.png')
            open(f, 'wb').close()                                         # only its existence is read (:173)
            payloads[f] = png[b]
            seq.paths_to_forward_flow.append(f)
        with np.errstate(invalid='ignore'):
            batch = sequence_collate_fn([seq.get_data_sample(b) for b in range(B)])
    events = batch['events'].numpy()
    flow, valid = batch['forward_flow'].numpy(), batch['flow_valid'].numpy()
    assert events.dtype == np.float32 and flow.dtype == np.float32 and valid.dtype == np.bool_
    assert flow.shape == (B, 2, K.H, K.W) and valid.shape == (B, K.H, K.W)
    ref_ev, ref_np = K.reference_events(m, x, y, t, p, counts, K.H, K.W, K.NB)
    assert np.array_equal(events, ref_ev) and int(batch['num_pos_events']) == ref_np          # the restatement the GPU tests lean on
    d_flow, d_valid = K.decode(png)
    assert np.array_equal(flow, d_flow) and np.array_equal(valid, d_valid)
    kept = sum(int((events[b, :, 5] == 1).sum()) for b in range(B))
    assert 0 < kept < int(counts.sum())
    path = os.path.join(args.out, 'g20_dsec_sample.npz')
    save_npz(path, dict(rectify_map=m, x=x.astype(np.uint16), y=y.astype(np.uint16), t=t, p=p.astype(np.uint8), counts=counts,
                        num_bins=np.int64(K.NB), events=events, num_pos_events=np.int64(batch['num_pos_events']),
                        voxel=batch['voxel'].numpy(), png16=png, forward_flow=flow, flow_valid=valid))
    print(f'g20_dsec_sample: {os.path.getsize(path)} B  events {events.shape}  kept {kept} of {int(counts.sum())}  valid share {valid.mean():.3f}')

    # ---- export: scripts/dsec_inference.py, imported from its file as it is
    spec = importlib.util.spec_from_file_location('dsec_inference_ref', os.path.join(args.ref, 'scripts', 'dsec_inference.py'))
    inf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inf)                                          # reference, unmodified
    out = {}
    for tag, (Bn, h, w) in (('', (2, 16, 24)), ('_odd', (2, 5, 7))):
        f = K.export_flow(Bn, h, w)
        got = []
        for b in range(Bn):
            scaled = inf.scale_optical_flow(torch.from_numpy(f[b].copy()), 60).numpy()          # :92-93
            inf.save_flow('unused.png', scaled)                                                  # :98
            got.append(written.pop()[1])
        got = np.stack(got)
        assert got.dtype == np.uint16 and got.shape == (Bn, h, w, 3) and not written
        assert np.array_equal(got, K.export(f)), tag
        share = float((np.hypot(f[:, 0].astype(np.float64), f[:, 1].astype(np.float64)) > 60).mean())
        assert 0.2 < share < 0.45, share
        out.update({'flow' + tag: f, 'png16' + tag: got})
        print(f'g20_dsec_export{tag}: {h}x{w}  share above 60 px {share:.3f}')
    path = os.path.join(args.out, 'g20_dsec_export.npz')
    save_npz(path, out)
    print(f'g20_dsec_export: {os.path.getsize(path)} B')


if __name__ == '__main__':
    main()
