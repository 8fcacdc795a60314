"""Cases and numpy / torch-CPU restatements for the DSEC rectification, flow decode and flow export (csrc/ingest.hip's map
source, csrc/dsec_io.hip) -- TEST INFRASTRUCTURE ONLY.  Every restatement cites the reference lines it restates; the fixtures
tests/golden/g20_dsec_*.npz (tools/gen_golden_dsec_io.py: the UNMODIFIED reference on the inputs built here) pin them, see
tests/test_dsec_io_host.py.  The same builders feed the generator and the tests, so a fixture's inputs can be rebuilt and checked."""
import os

import numpy as np
import torch


def load(name):
    """tests/golden/<name>.npz as a dict of arrays."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


H, W, NB = 48, 64, 5          # image of the ingest and payload cases, time bins
N_EVENTS, COUNTS = 4099, (4099, 1000, 257)          # N: no multiple of 4, several 256-row chunks


# ---- A: rectification ------------------------------------------------------------------------------------------------
def rectify_map(hs=H, ws=W, seed=2000):
    """[hs, ws, 2] float32, last axis (x_rect, y_rect): the identity plus a smooth distortion of up to +-3 px, so that rows
    leave a same-size image on all four sides, plus planted entries: 0.0, -0.0, exactly `ws` (dropped by `< width`), the float
    below it, NaN, +inf."""
    yy, xx = np.meshgrid(np.arange(hs, dtype=np.float64), np.arange(ws, dtype=np.float64), indexing='ij')
    g = np.random.default_rng(seed)
    a = g.uniform(0.6, 1.0, 4)
    dx = 3.0 * a[0] * np.sin(yy / hs * 2.3 + 0.4) * np.cos(xx / ws * 3.1 - 0.2) + 3.0 * (1 - a[0]) * ((xx / (ws - 1)) * 2 - 1)
    dy = 3.0 * a[1] * np.cos(yy / hs * 2.9 - 0.3) * np.sin(xx / ws * 2.1 + 0.5) + 3.0 * (1 - a[1]) * ((yy / (hs - 1)) * 2 - 1)
    # push the four borders outwards so that each side loses rows
    dx += -2.5 * np.exp(-xx / 2.0) + 2.5 * np.exp(-(ws - 1 - xx) / 2.0)
    dy += -2.5 * np.exp(-yy / 2.0) + 2.5 * np.exp(-(hs - 1 - yy) / 2.0)
    m = np.stack((xx + np.clip(dx, -3, 3), yy + np.clip(dy, -3, 3)), axis=-1).astype(np.float32)
    c = hs // 2
    m[c, 10, 0] = 0.0
    m[c, 11, 0] = -0.0
    m[c, 12, 0] = np.float32(ws)
    m[c, 13, 0] = np.nextafter(np.float32(ws), np.float32(0))
    m[c, 14, 0] = np.nan
    m[c, 15, 1] = np.inf
    m[c, 16, 1] = 0.0
    m[c, 17, 1] = -0.0
    return m


PLANTED = [(H // 2, x) for x in range(10, 18)]          # (y, x) of the planted map entries of the default map


def raw_window(hs=H, ws=W, seed=2010, n=N_EVENTS, counts=COUNTS):
    """The raw window of B samples as the DSEC slicer hands it over, padded to [B, n]: x, y sensor pixel indices (int32 here;
    uint16 in the h5 files), t int64 increasing microsecond stamps, p in {0, 1}; the first events of every sample visit the
    planted map entries, both polarities."""
    g = np.random.default_rng(seed)
    B = len(counts)
    x = np.zeros((B, n), np.int32); y = np.zeros((B, n), np.int32)
    t = np.zeros((B, n), np.int64); p = np.zeros((B, n), np.float32)
    for b, c in enumerate(counts):
        x[b, :c] = g.integers(0, ws, c); y[b, :c] = g.integers(0, hs, c)
        t[b, :c] = np.sort(g.choice(100000, c, replace=False)) + 51_000_000_000 + 100000 * b
        p[b, :c] = g.random(c) > 0.45
        if (hs, ws) == (H, W):
            for k, (py, px) in enumerate(PLANTED * 2):
                y[b, k], x[b, k], p[b, k] = py, px, float(k >= len(PLANTED))
    return x, y, t, p, np.asarray(counts, np.int32)


def gather(m, x, y):
    """loader.py:153,187-189: x_rect, y_rect = rectify_ev_map[y, x].T"""
    r = m[y, x]
    return r[..., 0], r[..., 1]


def reference_events(m, x, y, t, p, counts, height, width, num_bins):
    """loader.py:152-167 + 360-415 on the gathered coordinates: oracle.ingest_oracle restates exactly those lines."""
    from oracle import ingest_oracle as I
    samples = []
    for b, c in enumerate(counts):
        xr, yr = gather(m, x[b, :c], y[b, :c])
        with np.errstate(invalid='ignore'):
            samples.append(I.sample_events(xr, yr, t[b, :c], p[b, :c], height, width, num_bins))
    return I.collate(samples)


# ---- B: payload -> targets, error ------------------------------------------------------------------------------------
def payload(B, h, w, seed=2020):
    """[B, h, w, 3] uint16: x / y uniform over the whole range with planted 0, 32768, 65535; valid in {0, 1, 2, 255}."""
    g = np.random.default_rng(seed + 7 * h + w)
    png = g.integers(0, 65536, (B, h, w, 3)).astype(np.uint16)
    png[..., 2] = g.choice(np.array([0, 1, 2, 255], np.uint16), (B, h, w), p=[0.4, 0.3, 0.15, 0.15])
    for k, v in enumerate((0, 32768, 65535)):
        png[:, 0, k, 0] = v; png[:, 0, k, 1] = v; png[:, 0, k, 2] = 1
        png[:, 1, k, 0] = v; png[:, 1, k, 1] = 65535 - v
    return png


def decode(png):
    """loader.py:174-180 for a stack of payloads."""
    f16 = png.astype(np.float32)                                              # :174
    flow = np.zeros(png.shape[:-3] + (2,) + png.shape[-3:-1], dtype=np.float32)          # :175
    flow[..., 0, :, :] = (f16[..., 1] - 2**15) / 128.                          # :176
    flow[..., 1, :, :] = (f16[..., 0] - 2**15) / 128.                          # :177
    valid = f16[..., 2].astype(bool)                                          # :178
    return flow, valid


def prediction(flow_gt, seed=2030):
    """Half of the pixels a few px off the ground truth (so that 1PE / 2PE / 3PE lie strictly inside (0, 1)), the other half
    unrelated to it.  Why not all of them close: the ground truth of a uniform payload is ~130 px long, a prediction 1.5 px off
    it makes an angle of ~0.01 rad, and acos near 1 turns the fp32 rounding of the cosine (6e-8) into 1e-3 of such an angle --
    fp32 per-pixel arithmetic (the reference's own) then sits 3e-4 off float64 on AE, whatever the kernel does.  With the
    unrelated half (angles ~1 rad, where acos is well conditioned) carrying the AE sum, fp32 sits 1e-6 .. 4e-6 off float64 at
    48 x 64 and up to 1.3e-5 at 5 x 7 (70 pixels, hardly any averaging), inside FE_RTOL (the project's fp32 restatement on the
    CPU, oracle/flow_oracle.py, against flow_error64 below; the kernel gives the same figures)."""
    g = np.random.default_rng(seed)
    near = g.random(flow_gt.shape[:-3] + (1,) + flow_gt.shape[-2:]) < 0.5
    return np.where(near, flow_gt + g.normal(0, 1.5, flow_gt.shape), g.normal(0, 90, flow_gt.shape)).astype(np.float32)


FE_KEYS = ('EPE', '1PE', '2PE', '3PE', 'AE')
FE_RTOL = 2e-5          # the bound tests/test_gpu_flow.py holds calculate_flow_error to (fp32 per-pixel terms, acosf)


def flow_error64(flow_gt, flow_pred, event_mask=None, time_scale=None):
    """src/utils/flow.py:18-70 in float64 on the fp32 inputs (the reference runs the same lines in fp32)."""
    gt, pr = np.asarray(flow_gt, np.float64), np.asarray(flow_pred, np.float64)
    fm = ~np.isinf(gt[:, [0]]) & ~np.isinf(gt[:, [1]]) & (np.abs(gt[:, [0]]) > 0) & (np.abs(gt[:, [1]]) > 0)          # :35-40
    tm = fm if event_mask is None else np.logical_and(np.asarray(event_mask).reshape(fm.shape), fm)               # :42-46
    gm, pm = gt * tm, pr * tm                                                                                       # :48-49
    npts = tm.sum(axis=(1, 2, 3)) + 1e-5                                                                            # :51
    if time_scale is not None:                                                                                      # :53-55
        ts = np.asarray(time_scale, np.float64).reshape(len(gm), 1, 1, 1)
        gm, pm = gm * ts, pm * ts
    epe = np.sqrt(((gm - pm) ** 2).sum(axis=1))                                                                     # :57
    out = {'EPE': np.mean(epe.sum(axis=(1, 2)) / npts)}                                                             # :58
    for k in (1, 2, 3):
        out['%dPE' % k] = np.mean((epe > k).sum(axis=(1, 2)) / npts)                                                # :59-61
    u, v, ug, vg = pm[:, 0], pm[:, 1], gm[:, 0], gm[:, 1]                                                           # :63-64
    cs = (1.0 + u * ug + v * vg) / (np.sqrt(1 + u * u + v * v) * np.sqrt(1 + ug * ug + vg * vg))                    # :65-66
    out['AE'] = np.mean(np.arccos(np.clip(cs, -1, 1)).sum(axis=(1, 2)) / npts) * (180.0 / np.pi)                    # :67-69
    return out


# ---- C: export ---------------------------------------------------------------------------------------------------------
def export_flow(B, h, w, seed=2040):
    """[B, 2, h, w] float32 (y, x), N(0, 40^2) px (about 31 % of the pixels exceed 60), with planted pixels in row 0 / 1:
    (36, 48) of magnitude exactly 60 (not clamped), the next float above in one component (clamped), zeros, +-1e4, denormals."""
    g = np.random.default_rng(seed + 7 * h + w)
    f = (g.normal(0, 40, (B, 2, h, w))).astype(np.float32)
    up = np.nextafter(np.float32(48), np.float32(np.inf))
    planted = [(36, 48), (48, 36), (36, up), (up, 36), (-36, -48), (0, 0), (-0.0, 0.0), (1e4, -1e4), (-1e4, 3), (1e-40, -1e-42),
               (60, 0), (0, -60)]
    for k, (u, v) in enumerate(planted):
        f[:, 0, k // w, k % w] = u; f[:, 1, k // w, k % w] = v
    return f


def clamp(flow, max_magnitude=60.0):
    """scripts/dsec_inference.py:33-41 (scale_optical_flow) for [.., 2, h, w], torch on the CPU in fp32, line by line."""
    flow = torch.as_tensor(flow, dtype=torch.float32).clone()
    u, v = flow[..., 0, :, :], flow[..., 1, :, :]                             # :34
    magnitude = torch.sqrt(u**2 + v**2)                                       # :35
    exceed = magnitude > max_magnitude                                        # :36
    u[exceed] = (u[exceed] / magnitude[exceed]) * max_magnitude               # :38
    v[exceed] = (v[exceed] / magnitude[exceed]) * max_magnitude               # :39
    return torch.stack([u, v], dim=-3).numpy()                                # :41


def export(flow, max_magnitude=60.0):
    """dsec_inference.py:33-49 (scale_optical_flow + save_flow) -> [.., h, w, 3] uint16."""
    f = clamp(flow, max_magnitude)
    out = np.zeros(f.shape[:-3] + f.shape[-2:] + (3,), dtype=np.uint16)        # :46
    out[..., 1] = (f[..., 0, :, :] * 128 + 2**15).astype(np.uint16)            # :47  y-component
    out[..., 0] = (f[..., 1, :, :] * 128 + 2**15).astype(np.uint16)            # :48  x-component
    return out
