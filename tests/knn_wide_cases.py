"""Inputs and brute-force references shared by tests/test_knn_wide_host.py and tests/test_gpu_knn_wide.py: raw point sets of more
than 65535 trajectories per sample (the chunked KNN route, csrc/knn_wide.hip), the exact neighbour lists by (fp32 distance, index)
and a torch mirror of the chunk-merge rule."""
import torch

H, W, SP = 96, 128, 4                    # image and LUT cell: 24 x 32 = 768 queries per (sample, bin)
# (n, K, seed, nb, B): the point sets the GPU file holds against the oracle; tests/test_knn_wide_host.py proves that none of their
# queries has a neighbour set that depends on rounding (fp32 and fp64 brute force agree)
FIXTURES = {'n65536_k4': (65536, 4, 1, 3, 1), 'n70001_k32': (70001, 32, 2, 3, 1), 'n131072_k32': (131072, 32, 3, 2, 1),
            'n65536_k4_b2': (65536, 4, 4, 2, 2)}


def query_points():
    """Cell centres (y, x) [768, 2], focus.py:116-126."""
    off = SP / 2 - 0.5
    gy, gx = torch.meshgrid(torch.arange(0, H, SP, dtype=torch.float32) + off, torch.arange(0, W, SP, dtype=torch.float32) + off, indexing='ij')
    return torch.stack((gy, gx), -1).reshape(-1, 2)


def raw_trajectories(n, T, nb, seed, B=1):
    """[B, T + nb, n, 2] (y, x), reference rows first: a new uniform draw over the image and 4 px around it for every row of every
    sample.  A sample's nb mid-time rows are drawn before its T reference rows, so the point sets the search sees -- and with them
    the neighbour sets -- do not depend on T."""
    g = torch.Generator().manual_seed(seed)
    ext = torch.tensor([H + 8., W + 8.])
    out = []
    for _ in range(B):
        rows = [torch.rand(n, 2, generator=g) * ext - 4 for _ in range(nb + T)]
        out.append(torch.stack(rows[nb:] + rows[:nb]))
    return torch.stack(out)


def fixture(name, T=1):
    n, K, seed, nb, B = FIXTURES[name]
    return raw_trajectories(n, T, nb, seed, B), K


def duplicate_pairs(n, chunk_starts):
    """(query, a, b) with a < b: the points a and b are put ON the centre of cell `query` (distance 0), so that they are its two
    nearest and only the index ranks them.  One pair straddles every chunk boundary (lo - 1, lo), one is (0, n - 1)."""
    pairs = [(lo - 1, lo) for lo in chunk_starts[1:-1]] + [(0, n - 1)]
    return [((97 * j + 5) % 768, a, b) for j, (a, b) in enumerate(pairs)]


def with_duplicates(traj, chunk_starts):
    """The same points with the exact duplicates of duplicate_pairs in every row: ties that only the index decides, with the two
    members in different chunks."""
    t = traj.clone()
    q = query_points()
    for qi, a, b in duplicate_pairs(t.shape[2], chunk_starts):
        t[:, :, a] = t[:, :, b] = q[qi]
    return t


def chunk_starts(n, chunk):
    """ops.knn_chunk_starts, restated: ceil(n / chunk) contiguous chunks of near-equal length."""
    nc = -(-n // chunk)
    base, rem = divmod(n, nc)
    s = [0]
    for c in range(nc):
        s.append(s[-1] + base + (1 if c < rem else 0))
    return s


def distances(q, pts, norm='l2', dtype=torch.float32):
    """[Q, n] in the operand order of focus.py:132-135: (grid - traj) ** 2 summed y then x, or abs."""
    q, pts = q.to(dtype), pts.to(dtype)
    dy, dx = q[:, None, 0] - pts[None, :, 0], q[:, None, 1] - pts[None, :, 1]
    return dy * dy + dx * dx if norm == 'l2' else dy.abs() + dx.abs()


def ordered_knn(d, K, slack=8):
    """The K nearest per row of d [Q, n] as ORDERED lists by (distance, index) -- the project's tie rule: the lowest index wins --
    -> (idx [Q, K] int64, dist [Q, K]).  topk picks K + slack candidates (its tie order is undefined), which are then ordered by
    (distance, index); a row whose ties at the last candidate could reach into the first K goes through a full stable sort."""
    n = d.shape[1]
    m = min(n, K + slack)
    dv, di = torch.topk(d, m, dim=1, largest=False, sorted=True)
    o = torch.sort(di, dim=1, stable=True).indices                   # by index ...
    di, dv = di.gather(1, o), dv.gather(1, o)
    o = torch.sort(dv, dim=1, stable=True).indices                   # ... then, stably, by distance
    di, dv = di.gather(1, o), dv.gather(1, o)
    if m < n:
        unsure = dv[:, K - 1] == dv[:, m - 1]                        # ties beyond the candidates: topk may have dropped a lower index
        for r in torch.nonzero(unsure).flatten().tolist():
            sv, si = torch.sort(d[r], stable=True)
            di[r, :K], dv[r, :K] = si[:K], sv[:K]
    return di[:, :K], dv[:, :K]


def brute_knn(pts, K, norm='l2', dtype=torch.float32, q_chunk=256):
    """ordered_knn of all points [n, 2] for the 768 cell centres, computed on the device of `pts`."""
    q = query_points().to(pts.device)
    out = [ordered_knn(distances(q[s:s + q_chunk], pts, norm, dtype), K) for s in range(0, q.shape[0], q_chunk)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def chunk_merge_knn(pts, K, starts, norm='l2'):
    """Mirror of the chunked route: the K nearest of every contiguous chunk by (fp32 distance, index), then the K smallest of their
    union by (distance, global index)."""
    ci, cd = [], []
    for lo, hi in zip(starts[:-1], starts[1:]):
        i, d = brute_knn(pts[lo:hi], K, norm)
        ci.append(i + lo); cd.append(d)
    ci, cd = torch.cat(ci, 1), torch.cat(cd, 1)                      # [Q, C * K]
    o = torch.sort(ci, dim=1, stable=True).indices
    ci, cd = ci.gather(1, o), cd.gather(1, o)
    o = torch.sort(cd, dim=1, stable=True).indices
    return ci.gather(1, o)[:, :K]


def oracle_lut(traj, T, K, norm='l2', scheme='mean', want_next=False, dtype=torch.float64):
    """oracle.focus_oracle.interpolate_flow (focus.py:115-180) with the selection by brute_knn -- ranked in fp32 like the reference,
    topk instead of a full sort of every distance row -- and the interpolation in `dtype`: float32 is the oracle bit for bit
    (tests/test_knn_wide_host.py), float64 the oracle without its own rounding.  traj [B, T + nb, n, 2]; differentiable in traj.
    -> (flow_lut [B, nb, 24, 32, T, 2], flow_next [B, nb - 1, 24, 32, 1, 2] or None, idx [B, nb, 768, K])."""
    B, nb = traj.shape[0], traj.shape[1] - T
    q = query_points().to(dtype)
    tj = traj.to(dtype)
    lut, nxt, idx_all = [], [], []
    for b in range(B):
        for t in range(nb):
            idx, _ = brute_knn(traj[b, T + t].detach(), K, norm)
            f = tj[b, :T].permute(1, 0, 2) - tj[b, T + t][:, None, :]               # [n, T, 2]  focus.py:140-141
            g = f[idx]                                                             # [Q, K, T, 2]
            if K == 1 or scheme == 'mean':
                val = g.mean(1)
            else:
                diff = q[:, None, :] - tj[b, T + t].detach()[idx]
                dk = (diff ** 2).sum(-1) if norm == 'l2' else diff.abs().sum(-1)
                wgt = 1 / (dk + 1e-9)                                              # focus.py:158-162 (no grad)
                wgt = wgt / wgt.sum(1, keepdim=True)
                val = (wgt[..., None, None] * g).sum(1)
            lut.append(val)
            idx_all.append(idx)
            if want_next and t < nb - 1:
                nxt.append((tj[b, T + t + 1] - tj[b, T + t])[idx].mean(1))          # focus.py:171-175
    hq, wq = H // SP, W // SP
    flow_lut = torch.stack(lut).reshape(B, nb, hq, wq, T, 2)
    flow_next = torch.stack(nxt).reshape(B, nb - 1, hq, wq, 1, 2) if want_next else None
    return flow_lut, flow_next, torch.stack(idx_all).reshape(B, nb, hq * wq, K)
