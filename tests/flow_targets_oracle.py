"""Restatement of the ground-truth flow targets (utils.flow_targets, csrc/flow_targets.hip) in numpy: the formulas of the reference's
loaders (EVIMO2 src/loader/evimo2/datasubset.py:171-188, MultiFlow src/loader/multiflow/sample.py:108-139) written out operation
by operation, in fp32 (what torch's CPU kernels and the HIP kernel compute) and in float64 (the yardstick: the same formulas on the
fp32 inputs with the fp32 source indices and weights, every product and sum in float64).  Own code, no reference text."""
import numpy as np

F32 = np.float32


def src_half_pixel(size, out):
    """F.interpolate(mode='bilinear', align_corners=False) along one axis: (i0, i1, lam fp32) for the `out` output indices."""
    scale = F32(size) / F32(out)
    j = np.arange(out, dtype=F32)
    r = np.maximum(scale * (j + F32(0.5)) - F32(0.5), F32(0))
    i0 = np.minimum(np.floor(r).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    lam = np.clip(r - i0.astype(F32), F32(0), F32(1)).astype(F32)
    return i0, i1, lam


def src_aligned(size, out):
    """F.interpolate(mode='bilinear', align_corners=True) along one axis (out >= 2)."""
    scale = F32(size - 1) / F32(out - 1)
    r = scale * np.arange(out, dtype=F32)
    i0 = np.minimum(r.astype(np.int64), size - 1)
    i1 = np.where(i0 < size - 1, i0 + 1, i0)
    lam = np.clip(r - i0.astype(F32), F32(0), F32(1)).astype(F32)
    return i0, i1, lam


def src_nearest(size, out):
    """F.interpolate(mode='nearest') along one axis: min(floor(j * fp32(size / out)), size - 1)."""
    scale = F32(size) / F32(out)
    return np.minimum(np.floor(np.arange(out, dtype=F32) * scale).astype(np.int64), size - 1)


def blend(img, ys, xs, dtype):
    """img [..., H, W] -> [..., Ho, Wo]: columns blended first, rows last, every operation in `dtype`."""
    (y0, y1, ly), (x0, x1, lx) = ys, xs
    img = img.astype(dtype)
    lx, ly = lx.astype(dtype), ly.astype(dtype)[:, None]
    one = dtype(1)
    top = (one - lx) * img[..., y0[:, None], x0[None, :]] + lx * img[..., y0[:, None], x1[None, :]]
    bot = (one - lx) * img[..., y1[:, None], x0[None, :]] + lx * img[..., y1[:, None], x1[None, :]]
    return (one - ly) * top + ly * bot


def evimo2(raw, out_size, id_mask=None, dtype=F32):
    """raw [B, S, 2, H, W] fp32 with NaN -> (flow [B, S, 2, Ho, Wo] in `dtype`, flow_valid [B, S, Ho, Wo] bool, id [B, Ho, Wo] fp32 or
    None, x_scale, y_scale)."""
    raw = np.asarray(raw, dtype=F32)
    H, W = raw.shape[-2:]
    Ho, Wo = out_size
    valid_src = ~np.isnan(raw[:, :, 0]) & ~np.isnan(raw[:, :, 1])
    zeroed = np.where(np.isnan(raw), F32(0), raw)
    with np.errstate(invalid='ignore', over='ignore'):
        flow = blend(zeroed, src_half_pixel(H, Ho), src_half_pixel(W, Wo), dtype)
        flow[:, :, 0] *= dtype(F32(Wo / W))          # the Python float, rounded to fp32 by the multiply
        flow[:, :, 1] *= dtype(F32(Ho / H))
    ny, nx = src_nearest(H, Ho), src_nearest(W, Wo)
    valid = valid_src[:, :, ny[:, None], nx[None, :]]
    ids = None if id_mask is None else np.asarray(id_mask).astype(F32)[:, ny[:, None], nx[None, :]]
    return flow, valid, ids, Wo / W, Ho / H


def multiflow(raw, dtype=F32):
    """raw [B, S, H, W, 2] fp32 -> flow [B, S, 2, H // 2, W // 2] in `dtype`: no NaN treatment, no mask."""
    raw = np.moveaxis(np.asarray(raw, dtype=F32), -1, 2)
    H, W = raw.shape[-2:]
    with np.errstate(invalid='ignore', over='ignore'):
        return blend(raw, src_aligned(H, H // 2), src_aligned(W, W // 2), dtype) * dtype(0.5)


def torch_chain_evimo2(raw, out_size, id_mask=None):
    """The loader's operator chain with torch's own operators (any device): what the restatement restates."""
    import torch
    import torch.nn.functional as F
    B, S = raw.shape[:2]
    valid = ~torch.isnan(raw[:, :, 0]) & ~torch.isnan(raw[:, :, 1])
    flow = raw.clone()
    flow[torch.isnan(flow)] = 0.
    flow = F.interpolate(flow.flatten(0, 1), size=list(out_size), mode='bilinear', align_corners=False).unflatten(0, (B, S))
    valid = F.interpolate(valid.float(), size=list(out_size), mode='nearest').bool()
    ids = None if id_mask is None else F.interpolate(id_mask.float()[:, None], size=list(out_size), mode='nearest')[:, 0]
    flow[:, :, 0] *= out_size[1] / raw.shape[-1]
    flow[:, :, 1] *= out_size[0] / raw.shape[-2]
    return flow, valid, ids


def check_flow(label, out, flow64, err_ref):
    """The tolerance rule: max|out - flow64| <= 2 * err_ref (NaN must meet NaN); the figure is printed before it is asserted."""
    out, flow64 = np.asarray(out, dtype=np.float64), np.asarray(flow64, dtype=np.float64)
    assert out.shape == flow64.shape, (label, out.shape, flow64.shape)
    nan = np.isnan(flow64)
    assert np.array_equal(np.isnan(out), nan), label
    err = float(np.max(np.abs(np.where(nan, 0.0, out) - np.where(nan, 0.0, flow64))))
    print(f'{label}: max|out - flow64| = {err:.4g}  err_ref = {err_ref:.4g}  ratio {err / err_ref if err_ref else float("nan"):.3f}')
    assert err <= 2.0 * err_ref, (label, err, err_ref)
    return err
