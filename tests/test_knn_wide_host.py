"""CPU-only checks behind the chunked KNN route of more than 65535 trajectories per sample (csrc/knn_wide.hip, ops.knn_wide_fwd):
the rule the route rests on -- the K nearest of n points are the K smallest, by (distance, index), of the union of the K nearest of
every contiguous index chunk -- against brute force with the lowest-index tie rule, and the fixtures of tests/test_gpu_knn_wide.py:
none of their queries may have a neighbour set that depends on rounding."""
import ctypes

import pytest
import torch

import knn_wide_cases as KC


def test_ordered_knn_is_the_oracles_stable_sort():
    """The topk-based brute force of knn_wide_cases is what the oracle's stable sort gives, exact ties included."""
    from oracle import focus_oracle as O
    t = KC.with_duplicates(KC.raw_trajectories(3000, 1, 0, seed=5), [0, 1000, 2000, 3000])[0, 0]
    t[100:140] = t[100]                                              # forty points at one place: more ties than topk's slack
    for norm in ('l2', 'l1'):
        for K in (1, 4, 32):
            want, _ = O.knn_indices(t, KC.query_points(), K, norm)
            got, _ = KC.brute_knn(t, K, norm)
            assert torch.equal(got, want), (norm, K)


_SETS = {}


def _points(n, dup):
    key = (n, dup)
    if key not in _SETS:
        t = KC.raw_trajectories(n, 1, 0, seed=n % 97)
        if dup:
            t = KC.with_duplicates(t, KC.chunk_starts(n, 65535))
        _SETS[key] = (t[0, 0], KC.brute_knn(t[0, 0], 32)[0])         # (the lists of K = 1 and 4 are prefixes of the K = 32 list)
    return _SETS[key]


@pytest.mark.parametrize('K', [1, 4, 32])
@pytest.mark.parametrize('n,dup', [(65536, False), (65537, False), (131072, False), (131072, True)])
def test_chunk_merge_rule_is_exact(n, dup, K):
    """Chunks of at most 65535 points (two, two, three); the duplicated input has points lo - 1 and lo of every chunk boundary and
    points 0 and n - 1 at the same place: the index alone decides, across chunks."""
    pts, want = _points(n, dup)
    starts = KC.chunk_starts(n, 65535)
    assert len(starts) - 1 == (3 if n == 131072 else 2) and max(b - a for a, b in zip(starts, starts[1:])) <= 65535
    got = KC.chunk_merge_knn(pts, K, starts)
    assert torch.equal(got, want[:, :K])
    if dup:
        # the ties are really there: both members of every pair lead their query's list, the lower index first
        for qi, a, b in KC.duplicate_pairs(n, starts):
            assert want[qi, :2].tolist() == [a, b] and got[qi, 0] == a


@pytest.mark.parametrize('name', sorted(KC.FIXTURES))
def test_gpu_fixtures_have_no_rounding_ambiguous_neighbour(name):
    """fp32 and fp64 brute force pick the same K neighbours for every query of every bin of every sample: 0 differing queries (a
    seed that had one would be replaced, the cap stays).  Measured, smallest relative gap between the K-th and the (K + 1)-th fp64
    distance: n65536_k4 2 304 queries 1.6e-5, n65536_k4_b2 3 072 queries 6.5e-5, n70001_k32 2 304 queries 1.1e-6, n131072_k32
    1 536 queries 2.2e-5; an fp32 distance of these sizes is good to about 1e-7."""
    traj, K = KC.fixture(name)
    nb = traj.shape[1] - 1
    differing, queries, gap = 0, 0, float('inf')
    for b in range(traj.shape[0]):
        for t in range(nb):
            pts = traj[b, 1 + t]
            i32, _ = KC.brute_knn(pts, K)
            i64, d64 = KC.brute_knn(pts, K + 1, dtype=torch.float64)
            differing += int((torch.sort(i32, 1).values != torch.sort(i64[:, :K], 1).values).any(1).sum())
            queries += i32.shape[0]
            gap = min(gap, float(((d64[:, K] - d64[:, K - 1]) / d64[:, K]).min()))
    print(f'{name}: {queries} queries, {differing} differing, min relative gap K-th to (K+1)-th {gap:.2e}')
    assert differing == 0, (name, differing, gap)


@pytest.mark.parametrize('T,scheme,norm,want_next', [(1, 'mean', 'l2', True), (1, 'iwd', 'l1', True), (3, 'iwd', 'l2', False), (3, 'mean', 'l1', False)])
def test_oracle_lut_in_float32_is_the_oracle(T, scheme, norm, want_next):
    """knn_wide_cases.oracle_lut replaces the oracle's full sort by topk and nothing else: bit for bit its LUT, flow_to_next and
    neighbour lists, duplicates included (n small enough for the oracle's sort)."""
    from oracle import focus_oracle as O
    traj = KC.with_duplicates(KC.raw_trajectories(5000, T, 2, seed=9, B=2), [0, 2500, 5000])
    want = O.interpolate_flow(traj[:, :T], traj[:, T:], (KC.H, KC.W), KC.SP, 4, norm, scheme, want_next, return_idx=True)
    got = KC.oracle_lut(traj, T, 4, norm, scheme, want_next, dtype=torch.float32)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert (got[1] is None and want[1] is None) or torch.equal(got[1], want[1])


def test_chunk_starts_of_the_binding(monkeypatch):
    """ops.knn_chunk_starts: ceil(n / KNN_CHUNK) contiguous chunks of near-equal length, each of at least K points; the route starts
    at 65536 points with the shipped chunk; the limits are ValueErrors."""
    from motionpriorcmax_amd import ops
    assert ops.KNN_CHUNK == 65535 and not ops.knn_is_wide(65535) and ops.knn_is_wide(65536)
    for n in (65536, 65537, 70001, 131071, 131072, 307200):
        s = ops.knn_chunk_starts(n, 32)
        assert s == KC.chunk_starts(n, 65535) and s[0] == 0 and s[-1] == n
        lens = [b - a for a, b in zip(s, s[1:])]
        assert len(lens) == -(-n // 65535) and max(lens) - min(lens) <= 1 and max(lens) <= 65535
    monkeypatch.setattr(ops, 'KNN_CHUNK', 16384)
    assert ops.knn_chunk_starts(40000, 32) == [0, 13334, 26667, 40000] and ops.knn_is_wide(40000)
    monkeypatch.setattr(ops, 'KNN_CHUNK', 16)
    with pytest.raises(ValueError, match='num_knn=32'):
        ops.knn_chunk_starts(1000, 32)                               # chunks of 15 points cannot hold K = 32
    with pytest.raises(ValueError, match='at most 64 chunks'):
        ops.knn_chunk_starts(2000, 4)
    monkeypatch.setattr(ops, 'KNN_CHUNK', 70000)
    with pytest.raises(ValueError, match='KNN_CHUNK'):
        ops.knn_chunk_starts(80000, 4)


def test_wide_entry_points_check_their_arguments_on_the_host():
    """The three exports answer argument errors by code, before any launch: nulls, n above 2^22, more than 64 chunks, chunks that
    do not cover [0, n) or hold fewer than K points, and a chunks x K product the merge kernel's LDS cannot hold."""
    from motionpriorcmax_amd import _lib as C
    L = C.lib()

    def shape(n, K=4):
        return C.Shape(B=1, M=0, Mp=0, nb=2, T=1, H=96, W=128, sp=4, hq=24, wq=32, n=n, K=K, flags=0)
    s = shape(70000)
    assert L.mpc_knn_wide_workspace_bytes(ctypes.byref(s)) == 256 + 3 * 70000 * 2 * 8
    assert L.mpc_knn_wide_workspace_bytes(ctypes.byref(shape((1 << 22) + 1))) == C.E_UNSUPPORTED
    assert L.mpc_knn_merge_fwd(ctypes.byref(s), None, None, None, 2, None, None, None, None) == C.E_NULL
    assert L.mpc_knn_idx_bwd(ctypes.byref(s), None, None, None, None, None, None, None) == C.E_NULL
    p = ctypes.c_void_p(256)                                         # never dereferenced: every call below fails its checks first

    def merge(s, starts):
        arr = (ctypes.c_int32 * len(starts))(*starts)
        return L.mpc_knn_merge_fwd(ctypes.byref(s), p, p, arr, len(starts) - 1, p, p, p, None)
    assert merge(s, [0, 35000, 69999]) == C.E_SHAPE and b'cover' in L.mpc_last_error_string()
    assert merge(s, [0, 2, 70000]) == C.E_SHAPE                      # a chunk of 2 < K points (and one of more than 65535)
    assert merge(s, [0, 4464, 70000]) == C.E_SHAPE                   # a chunk of 65536 points: 65535 is the most
    assert merge(shape(4 << 20), [(4 << 20) * c // 65 for c in range(66)]) == C.E_UNSUPPORTED and b'64 chunks' in L.mpc_last_error_string()
    assert merge(shape((1 << 22) + 1), [0, 1 << 21, (1 << 22) + 1]) == C.E_UNSUPPORTED
    assert merge(shape(1 << 21, K=128), [(1 << 21) * c // 64 for c in range(65)]) == C.E_UNSUPPORTED and b'LDS' in L.mpc_last_error_string()
