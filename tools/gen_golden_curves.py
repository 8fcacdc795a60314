#!/usr/bin/env python3
"""Fixtures g21_curves_<case>.npz for the reference's other two RAFT-spline curve types (utils.trajectories_from_curves,
utils.flows_from_curves, utils.curve_basis, CorrLookup.lookup_curves, trajectory_val_metrics(curve_type=...)): the UNMODIFIED
reference's PolynomialCurves / LearnedCurves (src/models/raft_spline/curves/polynomial.py, learned.py, base.py) with the basis
network of src/modules/raft_spline.py:29-34 (1-64-64-d, ReLU), and for the lookup its CorrComputation /
CorrBlockParallelMultiTarget (corr.py), in fp32, beside a float64 evaluation of the formulas written out below and the measured
distance between the two -- the tests derive their tolerances from it.

    python tools/gen_golden_curves.py --ref PATH_TO_REFERENCE [--out tests/golden]

As tools/gen_golden_cvx.py: oracle/stubs stands in for the third-party packages the reference imports, the reference's own files
are imported as they are, and only DATA is written.  Deterministic (seeded, one thread): a second run reproduces the files bit
for bit.

Head cases (poly1, poly3, learned1, learned3, learned16, learned10) hold
  curve_type, params [B, 2d, h, w], mask [B, 576, h, w], times [8], tile, scale, g [B, 8, n, 2], flow_times; g_plain [B, 8, h * w, 2]
  net_<i>                      LEARNED: the network's parameters in `parameters()` order (W1, b1, W2, b2, W3, b3)
  basis, basis64               the [8, d] matrix the reference evaluates (list call) / its float64 evaluation
  traj, flows, grad_params, grad_mask (+ ..64, err_..)        create_upsampled(mask).get_flow_from_reference(list) at the tile centres
  traj_plain, grad_params_plain (+ ..64, err_..)              the curves of params on their own grid (tile centres of h*tile x w*tile)
  LEARNED: grad_basis, grad_basis_plain (retain_grad on the network's output), grad_net_<i>, grad_net_plain_<i> (+ ..64, err_..)
           S_grad_basis, S_grad_basis_plain [8, d]   float64 sum of the absolute addends of every grad_basis element, N_.. their count
           S_grad_net_<i>, S_grad_net_plain_<i>      sum over (t, j) of |d basis[t, j] / d theta| * S_grad_basis[t, j]
  learned3 also: val_gt [B, 8, 2, H, W], val_valid, val_event_mask, val_flows [8, B, 2, H, W] = the upsampled curve evaluated once
           per SCALAR timestamp as validation_step does (raft_spline.py:134-154: the shortcuts of base.py:98-106 at 0 and 1),
           val_flows64, err_val_flows, basis_val64 (the matrix with the two shortcut rows)
Lookup cases (corr_a, corr_b: the shapes of g16_corr_a / _b; corr_c: 9 x 11 = 99 pixels, two workgroups of 64 queries per sample), LEARNED:
  fmap1, fmap2, num_levels, radius, params, times, g, net_<i>, basis, basis64
  out, grad_params, grad_basis, grad_net_<i> (+ ..64, err_..), S_grad_basis, N_grad_basis, S_grad_net_<i>
The float64 results keep 29 significant bits, the logits lie on a grid of 1/16 and the feature maps on one of 1/4 (every pyramid
level exact in fp32), as in g13 / g16."""
import argparse
import copy
import math
import os
import sys

import numpy as np

TIMES = [0.41, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0, 1.0]          # t_ref, five bin mid-times, and the two ends base.py:102-106 special-cases
FLOW_TIMES = [0, 3, 7]
HEAD_CASES = [  # name, curve type, B, d, (h, w), tile, scale
    ('poly1', 'POLYNOMIAL', 2, 1, (2, 3), 4, 1.0),
    ('poly3', 'POLYNOMIAL', 2, 3, (2, 3), 4, 8.0),
    ('learned1', 'LEARNED', 2, 1, (2, 3), 4, 1.0),
    ('learned3', 'LEARNED', 2, 3, (2, 3), 4, 8.0),
    ('learned16', 'LEARNED', 1, 16, (4, 4), 16, 1.0),     # the register-heaviest instantiation
    ('learned10', 'LEARNED', 1, 10, (3, 33), 4, 8.0),     # 6 x 66 = 396 centres: two workgroups, partials are summed
]
MARGIN = 2.0 ** -10
CORR_CASES = [  # name, B, D, (h, w), num_levels, d, radius, amplitude of the control points
    ('corr_a', 2, 4, (6, 8), [1, 2], 3, 4, 3.0),
    ('corr_b', 1, 16, (5, 7), [1, 1, 2], 10, 4, 3.0),
    ('corr_c', 2, 4, (9, 11), [2, 1], 3, 2, 2.0),
]


def keep29(a):
    """float64 array with the low 24 mantissa bits cleared."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return (a.view(np.int64) & ~np.int64((1 << 24) - 1)).view(np.float64)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


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
    from src.models.raft_spline.curves import PolynomialCurves, LearnedCurves                   # reference, unmodified
    from src.models.raft_spline.corr import CorrComputation, CorrBlockParallelMultiTarget       # reference, unmodified
    from src.models.raft_spline.utils import coords_grid                                        # reference, unmodified
    from src import utils as rutils                                                             # reference, unmodified

    torch.set_num_threads(1)
    os.makedirs(args.out, exist_ok=True)
    largest = max(os.path.getsize(os.path.join(args.out, f)) for f in os.listdir(args.out) if f.startswith('g13_cvx_'))

    def make_net(d, seed):
        """The basis network of src/modules/raft_spline.py:29-34, default initialisation under a fixed seed."""
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(1, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, d))

    class Tap:
        """Keeps the output of the network's next call and asks autograd to retain its gradient (a forward hook: the reference's
        files stay as they are)."""

        def __init__(self, net):
            self.out = None
            self.handle = net.register_forward_hook(self)

        def __call__(self, module, inputs, output):
            output.retain_grad()
            self.out = output

    def basis64(ctype, times, d, net64):
        """The matrix in float64 from the fp32-rounded times (polynomial.py:55, learned.py:75): t^j, or the network in float64."""
        t = torch.tensor(times, dtype=torch.float64).float().double()
        if ctype == 'POLYNOMIAL':
            return t[:, None] ** torch.arange(1, d + 1, dtype=torch.float64)[None, :]
        return net64(t[:, None])

    def shortcut64(bm, times):
        bm = bm.clone()
        for i, t in enumerate(times):
            if t == 1:
                bm[i] = 0
                bm[i, -1] = 1
            if t == 0:
                bm[i] = 0
        return bm

    def upsample64(P, M):
        B, c2, h, w = P.shape
        H, W = 8 * h, 8 * w
        y, x = torch.arange(H), torch.arange(W)
        cy, sy, cx, sx = (y // 8)[:, None], (y % 8)[:, None], (x // 8)[None, :], (x % 8)[None, :]
        logits = M.view(B, 9, 8, 8, h, w)[:, :, sy, sx, cy, cx]                      # [B, 9, H, W]
        e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        wk = e / e.sum(dim=1, keepdim=True)
        P0 = torch.cat((torch.zeros(B, c2, 1, w, dtype=torch.float64), P, torch.zeros(B, c2, 1, w, dtype=torch.float64)), dim=2)
        P0 = torch.cat((torch.zeros(B, c2, h + 2, 1, dtype=torch.float64), P0, torch.zeros(B, c2, h + 2, 1, dtype=torch.float64)), dim=3)
        up = 0
        for k in range(9):
            up = up + wk[:, None, k] * 8 * P0[:, :, cy + k // 3, cx + k % 3]         # [B, 2d, H, W]
        return up

    def traj_of(flows, idx, pos):
        """flows [T, B, 2, H, W] (x, y), sampled at idx [n, 2] -> trajectories [B, T, n, 2] (y, x) from the start points pos."""
        at = flows[:, :, :, idx[:, 0], idx[:, 1]]
        return torch.stack((at[:, :, 1], at[:, :, 0]), dim=-1).permute(1, 0, 2, 3) + pos.to(flows.dtype)[None, None]

    def net_jacobian_abs_times(bm, params64, S):
        """sum over (t, j) of |d bm[t, j] / d theta| * S[t, j] per network parameter."""
        out = [torch.zeros_like(p) for p in params64]
        for t in range(bm.shape[0]):
            for j in range(bm.shape[1]):
                gs = torch.autograd.grad(bm[t, j], params64, retain_graph=True, allow_unused=True)
                for o, gth in zip(out, gs):
                    if gth is not None:
                        o += gth.abs() * S[t, j]
        return out

    def put(out, nm, r, f):
        r = r.detach().numpy() if hasattr(r, 'detach') else r
        f = keep29(f.detach().numpy() if hasattr(f, 'detach') else f)
        assert r.dtype == np.float32 and r.shape == f.shape, (nm, r.dtype, r.shape, f.shape)
        out[nm], out[nm + '64'] = r, f
        out['err_' + nm] = np.float64(np.abs(r.astype(np.float64) - f).max())

    def head_route(ctype, P, M, idx, pos, scale, g, net, times, d):
        """One route (M None: the curves of P on their own grid) -> {name: (fp32 reference, float64)} and the S sums."""
        res = {}
        # ---- the reference, fp32
        Pr = P.clone().requires_grad_(True)
        Mr = None if M is None else M.clone().requires_grad_(True)
        tap = Tap(net) if net is not None else None
        curve = PolynomialCurves(Pr) if ctype == 'POLYNOMIAL' else LearnedCurves(Pr, net)
        if Mr is not None:
            curve = curve.create_upsampled(Mr)
        flows = curve.get_flow_from_reference(list(times)) * scale
        traj = traj_of(flows, idx, pos)
        leaves = [Pr] + ([] if Mr is None else [Mr])
        if net is not None:
            for p in net.parameters():
                p.grad = None
            traj.backward(g, inputs=leaves + list(net.parameters()))
            ref = dict(traj=traj.detach(), flows=flows.detach()[FLOW_TIMES], grad_params=Pr.grad, grad_basis=tap.out.grad.clone(), basis=tap.out.detach().clone())
            for i, p in enumerate(net.parameters()):
                ref[f'grad_net_{i}'] = p.grad.clone()
            tap.handle.remove()
        else:
            gl = torch.autograd.grad(traj, leaves, g)
            ref = dict(traj=traj.detach(), flows=flows.detach()[FLOW_TIMES], grad_params=gl[0],
                       basis=torch.tensor(times, dtype=torch.float64).float()[:, None] ** torch.arange(1, d + 1)[None, :])
        if Mr is not None:
            ref['grad_mask'] = Mr.grad if net is not None else gl[1]
        # ---- float64
        P64 = P.double().requires_grad_(True)
        M64 = None if M is None else M.double().requires_grad_(True)
        net64 = None if net is None else copy.deepcopy(net).double()
        bm = basis64(ctype, times, d, net64)
        if net is not None:
            bm.retain_grad()
        up = P64 if M64 is None else upsample64(P64, M64)
        B = P.shape[0]
        upv = up.view(B, 2, d, *up.shape[-2:])
        flows64 = torch.einsum('bcjhw,tj->tbchw', upv, bm) * scale
        traj64 = traj_of(flows64, idx, pos)
        leaves64 = [P64] + ([] if M64 is None else [M64])
        params64 = [] if net is None else list(net64.parameters())
        traj64.backward(g.double(), inputs=leaves64 + params64 + ([bm] if net is not None else []), retain_graph=net is not None)
        f64 = dict(traj=traj64.detach(), flows=flows64.detach()[FLOW_TIMES], grad_params=P64.grad, basis=bm.detach())
        if M64 is not None:
            f64['grad_mask'] = M64.grad
        extra = {}
        if net is not None:
            f64['grad_basis'] = bm.grad
            for i, p in enumerate(params64):
                f64[f'grad_net_{i}'] = p.grad
            # grad_basis[t][j] = scale * sum_{b, n} (g.y * up.y[j] + g.x * up.x[j]): the sum of its absolute addends and their count
            at = upv.detach()[:, :, :, idx[:, 0], idx[:, 1]]                          # [B, 2 (x, y), d, n]
            gd = g.double()                                                           # [B, T, n, 2 (y, x)]
            S = scale * (torch.einsum('btn,bjn->tj', gd[..., 0].abs(), at[:, 1].abs()) + torch.einsum('btn,bjn->tj', gd[..., 1].abs(), at[:, 0].abs()))
            extra['S_grad_basis'] = S.numpy()
            extra['N_grad_basis'] = np.int64(2 * B * pos.shape[0])
            for i, s in enumerate(net_jacobian_abs_times(bm, params64, S)):
                extra[f'S_grad_net_{i}'] = s.numpy()
        return ref, f64, extra

    # ---------------------------------------------------------------- the output head
    for idx, (name, ctype, B, d, (h, w), tile, scale) in enumerate(HEAD_CASES):
        gen = torch.Generator().manual_seed(2100 + idx)
        P = torch.randn(B, 2 * d, h, w, generator=gen) * 0.5
        M = torch.round(torch.randn(B, 576, h, w, generator=gen) * 2.0 * 16.0) / 16.0
        pos = torch.nonzero(rutils.get_optical_flow_tile_mask((8 * h, 8 * w), tile))
        pos_plain = torch.nonzero(rutils.get_optical_flow_tile_mask((h * tile, w * tile), tile))
        g = torch.randn(B, len(TIMES), pos.shape[0], 2, generator=gen)
        g_plain = torch.randn(B, len(TIMES), h * w, 2, generator=gen)
        net = make_net(d, 2150 + idx) if ctype == 'LEARNED' else None
        out = dict(curve_type=np.asarray(ctype), params=P.numpy(), mask=M.numpy(), times=np.asarray(TIMES, dtype=np.float64), tile=np.int64(tile),
                   scale=np.float64(scale), g=g.numpy(), g_plain=g_plain.numpy(), flow_times=np.asarray(FLOW_TIMES, dtype=np.int64))
        if net is not None:
            for i, p in enumerate(net.parameters()):
                out[f'net_{i}'] = p.detach().numpy().copy()
        ref, f64, extra = head_route(ctype, P, M, pos, pos, scale, g, net, TIMES, d)
        for nm in ref:
            put(out, nm, ref[nm], f64[nm])
        out.update(extra)
        # the curves of params on their own grid: traj at the tile centres of the (h * tile) x (w * tile) image, n = h * w
        Pp_ref, Pp_64, Pp_extra = head_route(ctype, P, None, pos_plain // tile, pos_plain, scale, g_plain, net, TIMES, d)
        for nm in ('traj', 'grad_params') + (('grad_basis',) + tuple(f'grad_net_{i}' for i in range(6)) if net is not None else ()):
            r, f = Pp_ref[nm], Pp_64[nm]
            put(out, nm.replace('grad_net_', 'grad_net_plain_') if nm.startswith('grad_net_') else nm + '_plain', r, f)
        for k, v in Pp_extra.items():
            out[k.replace('S_grad_net_', 'S_grad_net_plain_') if k.startswith('S_grad_net_') else k + '_plain'] = v
        if name == 'learned3':
            # ---- what validation_step evaluates: once per SCALAR timestamp (np.float64 is a float: base.py:98)
            H, W = 8 * h, 8 * w
            with torch.no_grad():
                curve = LearnedCurves(P, net).create_upsampled(M)
                val = torch.stack([curve.get_flow_from_reference(ts) for ts in np.asarray(TIMES, dtype='float64')]) * scale
                net64 = copy.deepcopy(net).double()
                bmv = shortcut64(basis64(ctype, TIMES, d, net64), TIMES)
                val64 = torch.einsum('bcjhw,tj->tbchw', upsample64(P.double(), M.double()).view(B, 2, d, H, W), bmv) * scale
            put(out, 'val_flows', val, val64)
            out['basis_val64'] = bmv.numpy()
            out['val_gt'] = (val.permute(1, 0, 2, 3, 4) + torch.randn(B, len(TIMES), 2, H, W, generator=gen) * 2.0).numpy()
            out['val_valid'] = (torch.rand(B, len(TIMES), H, W, generator=gen) < 0.8).numpy()
            out['val_event_mask'] = (torch.rand(B, H, W, generator=gen) < 0.6).numpy()
        path = os.path.join(args.out, f'g21_curves_{name}.npz')
        save_npz(path, out)
        for nm in ('grad_mask', 'flows', 'traj'):                # too large: only the float64 tensor of the largest ones (err_X stays)
            if os.path.getsize(path) > largest:
                del out[nm]
                save_npz(path, out)
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
        print(f'g21_curves_{name}: {os.path.getsize(path)} B  n = {pos.shape[0]}  ' +
              '  '.join(f'{k} = {float(v):.3g}' for k, v in out.items() if k.startswith('err_')))

    # ---------------------------------------------------------------- the correlation lookup (LEARNED)
    def centres64(P, bm):
        B, c2, h, w = P.shape
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        flows = torch.einsum('bcjhw,tj->tbchw', P.view(B, 2, c2 // 2, h, w), bm)
        return torch.stack((xs, ys), dim=0)[None, None] + flows                               # [T, B, 2, h, w], (x, y)

    def formula64(levels, tix, r, coords):
        """out[b, e * K * K + i * K + j, y, x] = bilinear sample of levels[l][k][b * h * w + y * w + x] at
        (coords[t, b, 0, y, x] / 2^l + j - r, coords[t, b, 1, y, x] / 2^l + i - r), zero outside, per tap."""
        T, B, _, h, w = coords.shape
        K = 2 * r + 1
        off = torch.arange(-r, r + 1, dtype=torch.float64)
        out = []
        for l, (lv, ts) in enumerate(zip(levels, tix)):
            hl, wl = lv.shape[-2:]
            for k, t in enumerate(ts):
                px = (coords[t, :, 0] / 2 ** l)[..., None, None] + off[None, None, None, None, :]          # [B, h, w, 1, K]
                py = (coords[t, :, 1] / 2 ** l)[..., None, None] + off[None, None, None, :, None]          # [B, h, w, K, 1]
                x0, y0 = torch.floor(px).detach(), torch.floor(py).detach()
                fx, fy = px - x0, py - y0
                vol = lv[k].reshape(B * h * w, hl * wl)

                def tap(yi, xi):
                    yi, xi = yi.expand(B, h, w, K, K), xi.expand(B, h, w, K, K)
                    ok = (yi >= 0) & (yi < hl) & (xi >= 0) & (xi < wl)
                    idx = (yi.clamp(0, hl - 1) * wl + xi.clamp(0, wl - 1)).long().reshape(B * h * w, K * K)
                    return vol.gather(1, idx).reshape(B, h, w, K, K) * ok
                val = (tap(y0, x0) * ((1 - fx) * (1 - fy)) + tap(y0, x0 + 1) * (fx * (1 - fy)) +
                       tap(y0 + 1, x0) * ((1 - fx) * fy) + tap(y0 + 1, x0 + 1) * (fx * fy))
                out.append(val.reshape(B, h, w, K * K).permute(0, 3, 1, 2))
        return torch.cat(out, dim=1)

    for idx, (name, B, D, (h, w), nl, d, r, amp) in enumerate(CORR_CASES):
        n = len(nl)
        times = [(i + 1) / n for i in range(n)]                  # raft.py:169-176; the last is exactly 1.0 (a LIST: no shortcut)
        net = make_net(d, 2180 + idx)
        net64 = copy.deepcopy(net).double()
        for attempt in range(64):
            seed = 2200 + 100 * idx + attempt
            gen = torch.Generator().manual_seed(seed)
            f1 = torch.round(torch.randn(B, D, h, w, generator=gen) * 4.0) / 4.0
            f2 = torch.round(torch.randn(n, B, D, h, w, generator=gen) * 4.0) / 4.0
            P = torch.randn(B, 2 * d, h, w, generator=gen) * amp
            with torch.no_grad():
                bmd = basis64('LEARNED', times, d, net64)
                for _ in range(64):                              # the margin at integers: redraw the control points of the pixels that miss it
                    c = centres64(P.double(), bmd)
                    near = torch.zeros(B, h, w, dtype=torch.bool)
                    for l in range(max(nl)):
                        s = c / 2 ** l
                        near |= ((s - torch.round(s)).abs() < 2 * MARGIN).any(dim=2).any(dim=0)
                    if not bool(near.any()):
                        break
                    P = torch.where(near[:, None], torch.randn(B, 2 * d, h, w, generator=gen) * amp, P)
            K = 2 * r + 1
            g = torch.randn(B, sum(nl) * K * K, h, w, generator=gen)
            # ---- the reference, fp32
            block = CorrBlockParallelMultiTarget(corr_computation_events=CorrComputation(f1, f2, num_levels_per_target=list(nl)), radius=r)
            tix = [cd.target_indices.tolist() for cd in block._corr_pyramid]
            levels32 = [cd.corr.detach().clone() for cd in block._corr_pyramid]
            Pr = P.clone().requires_grad_(True)
            tap = Tap(net)
            for p in net.parameters():
                p.grad = None
            coords1 = coords_grid(B, h, w, Pr.device) + LearnedCurves(Pr, net).get_flow_from_reference(time=list(times))
            outr = block(coords1)
            outr.backward(g, inputs=[Pr] + list(net.parameters()))
            tap.handle.remove()
            ref = dict(out=outr.detach(), grad_params=Pr.grad, grad_basis=tap.out.grad.clone(), basis=tap.out.detach().clone())
            for i, p in enumerate(net.parameters()):
                ref[f'grad_net_{i}'] = p.grad.clone()
            # ---- float64
            P64 = P.double().requires_grad_(True)
            params64 = list(net64.parameters())
            for p in params64:
                p.grad = None
            bm = basis64('LEARNED', times, d, net64)
            bm.retain_grad()
            c64 = centres64(P64, bm)
            c64.retain_grad()
            out64 = formula64([lv.double() for lv in levels32], tix, r, c64)
            out64.backward(g.double(), inputs=[P64, bm, c64] + params64, retain_graph=True)
            f64 = dict(out=out64.detach(), grad_params=P64.grad, grad_basis=bm.grad, basis=bm.detach())
            for i, p in enumerate(params64):
                f64[f'grad_net_{i}'] = p.grad
            cd_ = c64.detach()
            margin = min(float(((cd_ / 2 ** l) - torch.round(cd_ / 2 ** l)).abs().min()) for l in range(max(nl)))
            c32 = coords1.detach().double()
            margin = min(margin, min(float(((c32 / 2 ** l) - torch.round(c32 / 2 ** l)).abs().min()) for l in range(max(nl))))
            zero = float((ref['out'] == 0).double().mean())
            if margin >= MARGIN and zero <= 0.75:
                break
        assert margin >= MARGIN and zero <= 0.75, (name, margin, zero)
        lvl0 = (f1.double().view(B, D, h * w).transpose(-1, -2) @ f2.double().view(n, B, D, h * w)) / math.sqrt(D)
        assert torch.equal(lvl0.view(levels32[0].shape), levels32[0].double()), name      # every level is exact in fp32
        # grad_basis[t][j] = sum_{b, pixel, axis} grad centre[t][b][axis] * params[b][axis][j]
        gc = c64.grad.abs()                                                               # [T, B, 2, h, w]
        S = torch.einsum('tbchw,bcjhw->tj', gc, P.double().abs().view(B, 2, d, h, w))
        arrays = dict(curve_type=np.asarray('LEARNED'), fmap1=f1.numpy(), fmap2=f2.numpy(), num_levels=np.asarray(nl, dtype=np.int64), radius=np.int64(r),
                      params=P.numpy(), times=np.asarray(times, dtype=np.float64), g=g.numpy(), seed=np.int64(seed))
        for i, p in enumerate(net.parameters()):
            arrays[f'net_{i}'] = p.detach().numpy().copy()
        for nm in ref:
            put(arrays, nm, ref[nm], f64[nm])
        arrays['S_grad_basis'] = S.numpy()
        arrays['N_grad_basis'] = np.int64(2 * B * h * w)
        for i, s in enumerate(net_jacobian_abs_times(bm, params64, S)):
            arrays[f'S_grad_net_{i}'] = s.numpy()
        path = os.path.join(args.out, f'g21_curves_{name}.npz')
        save_npz(path, arrays)
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
        print(f'g21_curves_{name}: seed {seed}  {os.path.getsize(path)} B  zero share of out {zero:.3f}  margin {margin:.3g}  ' +
              '  '.join(f'{k} = {float(v):.3g}' for k, v in arrays.items() if k.startswith('err_')))


if __name__ == '__main__':
    main()
