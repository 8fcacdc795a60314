"""numpy restatement of the loss-event ingest of the EVIMO2 and MultiFlow configurations -- a helper of the tests (no test in
here), pinned bit for bit by tests/golden/g14_window_*.npz (made by the unmodified reference: tools/gen_golden_window.py).

  evimo2_sample     reference src/loader/evimo2/datasubset.py:206-215.  Everything after the int64 stamps is FLOAT32 there:
                    `ts[-1] - flow_duration * 1e3` promotes an int64 0-dim tensor and a Python float to fp32, the comparison
                    with the int64 column then runs in fp32, and so do the normalisation and torch.searchsorted over the fp32
                    edges of torch.linspace.  Each step below is one fp32 operation.
  multiflow_sample  src/loader/multiflow/sample.py:224-236: float64 min/max normalisation, np.linspace edges, fp32 last.
  split / collate   datasubset.py:217-223, src/loader/multiflow/datasubset.py:149-156, src/modules/data_loading.py:14-47."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('g14_window_evimo2_split', 'g14_window_evimo2_single', 'g14_window_multiflow')


def load_window(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def evimo2_edges(num_bins):
    """datasubset.py:77: the fp32 edges as torch computes them on the CPU (they are not i / num_bins rounded to fp32)."""
    return torch.linspace(0, 1, int(num_bins) + 1).numpy()


def evimo2_sample(x, y, t_us, p, num_bins, flow_duration_ms):
    """-> [n_kept, 5] float32 columns (y, x, t, p, bin).  An empty window gives no rows (the reference raises on ts[-1])."""
    if len(t_us) == 0:
        return np.zeros((0, 5), np.float32)
    f32 = np.float32
    t = np.asarray(t_us, dtype=np.int64).astype(f32)                  # round to nearest
    ts_start = f32(t[-1] - f32(flow_duration_ms * 1e3))               # :208
    keep = t > ts_start                                               # :210 (strict)
    den = f32(t[-1] - ts_start)                                       # :211, ts_end - ts_start
    tn = ((t[keep] - ts_start) / den).astype(f32)                     # two fp32 operations
    bins = np.searchsorted(evimo2_edges(num_bins), tn, side='left') - 1          # :213
    bins[bins == -1] = 0                                              # :214
    col = lambda a: np.asarray(a)[keep].astype(f32)
    return np.stack((col(y), col(x), tn, col(p), bins.astype(f32)), axis=1)


def multiflow_sample(x, y, t_us, p, num_bins):
    """-> [n, 5] float32.  A window of one event divides 0 by 0, as the reference does (NaN time, bin = num_bins)."""
    if len(t_us) == 0:
        return np.zeros((0, 5), np.float32)
    t = np.asarray(t_us, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        t = (t - t.min()) / (t.max() - t.min())                       # :230-231 (float64)
    bins = np.searchsorted(np.linspace(0, 1, int(num_bins) + 1), t) - 1          # :232
    bins[bins == -1] = 0
    return np.column_stack((y, x, t, p, bins)).astype('float32')      # :235


def collate(samples, polarity_aware_batching):
    """samples: list of [n, 5] -> (events [B, M, 6], num_pos_events).  Without the split: one block, num_pos_events = -1."""
    if polarity_aware_batching:
        blocks = [(s[s[:, 3] == 1], s[s[:, 3] == 0]) for s in samples]
    else:
        blocks = [(s, s[:0]) for s in samples]
    max_pos = max(len(b[0]) for b in blocks)
    max_neg = max(len(b[1]) for b in blocks)
    out = np.zeros((len(samples), max_pos + max_neg, 6), dtype=np.float32)
    for b, (pos, neg) in enumerate(blocks):
        out[b, :len(pos), :5] = pos
        out[b, :len(pos), 5] = 1
        out[b, max_pos:max_pos + len(neg), :5] = neg
        out[b, max_pos:max_pos + len(neg), 5] = 1
    return out, (max_pos if polarity_aware_batching else -1)


def restate(dataset, x, y, t_us, p, counts, num_bins, flow_duration_ms=None, polarity_aware_batching=True):
    """The padded [B, N] arrays of `ingest_raw_events` -> (events, num_pos_events)."""
    rows = []
    for b, n in enumerate(int(c) for c in counts):
        a = (x[b, :n], y[b, :n], t_us[b, :n], p[b, :n])
        rows.append(evimo2_sample(*a, num_bins, flow_duration_ms) if dataset == 'evimo2' else multiflow_sample(*a, num_bins))
    return collate(rows, polarity_aware_batching)
