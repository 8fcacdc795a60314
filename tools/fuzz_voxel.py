"""Randomised differential test of the voxel-grid builder (`voxel_grids`: k_vox_bin, k_vox_accum<0 / 1 / 2>, k_vox_finalize, the
radix select k_vox_qhist / qscan / qnext / qclip, k_vox_stats, k_vox_norm over strip_buckets.h) against the float64 oracle
(`oracle.voxel_oracle.voxel_grid64`) over random small configurations: shape, batch, ragged counts, normalisation, quantile,
event placement.  Diagnostics; run on a GPU box:

    python tools/fuzz_voxel.py [n_cases] [seed]

Per case and sample the rule of tests/voxel_cases.py: max |gpu - f64| <= max(4 err32, 2^-22 max |f64|) + T 2^-30 m with err32 the
fp32 oracle's own distance from float64, no entry excused, entries that are zero in float64 +-0 on the device, nothing non-finite.
A case whose INPUTS break a cap (an entry within the raw bound of 0, or a non-zero status that differs between fp32 and float64)
is redrawn and counted; more than 1 redraw in 10 cases counts as bad.  The rare routes come round by the case index, not by luck
(see `draw_case`), every route is detected from the geometry, the per-bucket fills, the events and the oracle's ranks rather than claimed, and
the summary counts them: with 30 cases or more, a route that no case took counts as bad.

Measured on an MI355X with `40 25` (0 bad, 0 redrawn; every route taken: NS > 1 12, short last strip 8, spill 4, B > 1 19, empty
sample 4, q > 0 32, zero threshold 6, tied threshold 4, integer rank 5, wide sensor 4, integer coordinates 4, times outside 4):
worst ratio of a difference to its bound 0.499; 0.4 s for the 40 cases, oracle included.
With the kernels broken on purpose (arithmetic only, each in a build of its own; tests/test_gpu_voxel_cases.py + test_gpu_voxel.py
have 115 tests, this tool 40 cases):
  `(int)floorf(tn)` for `(int)tn`: the six 'time' cases and g8_voxel_e_time fail, nothing of test_gpu_voxel.py; fuzz cases 26, 36 (time).
  `>= k1` for `> k1` in k_vox_qclip: 24 case tests fail -- every q = 0.05 run of spill (mean_std), short_strip, wide, tiny_2x1x9 (and
    q = 0.125), tiny_3x5x7, time, ragged, nonfinite; the integer-rank and tied cases pass, as they must -- and three g8 fixtures;
    19 fuzz cases.
  statistics of k_vox_accum<1> without `if (v != 0.f)`: mean_std at q = 0 of spill, short_strip, wide, integer_ties, sparse, time,
    ragged, nonfinite, all_equal and g8_voxel_e_two_int fail; fuzz cases 10, 31, 37.
  `/ n` for `/ (n - 1.0)` in k_vox_finalize: all 24 mean_std case tests with more than one non-zero entry fail; 11 fuzz cases.
  sb_drain without the spilled runs for MODE == 1: spill with mean_std and max, the two run-to-run tests of those and the
    batch-against-alone test fail, nothing of test_gpu_voxel.py; fuzz cases 10, 20 (spill).
Under the bounds-checked build (-DMPC_BOUNDS) the same tests, tests/test_gpu_repr.py and this tool pass with mpc_bounds_check() 0.
"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))          # voxel_cases: the generators, the geometry and the bound the suite uses
import torch

ROUTES = ('NS > 1', 'short last strip', 'spill', 'B > 1', 'empty sample', 'q > 0', 'zero threshold', 'tied threshold',
          'integer rank', 'wide sensor', 'integer coordinates', 'times outside [first, last]')
KINDS = ('spill', 'short', 'wide', 'integer', 'sparse', 'intrank', 'time', 'random', 'random', 'ragged')
SHORT_HW = ((5, 2400), (7, 2400), (10, 2400), (11, 2400), (7, 1920), (11, 1920))
INTRANK_SHAPES = ((3, 5, 7), (1, 5, 5), (1, 3, 3), (3, 11, 1), (1, 7, 7), (3, 3, 9))        # (C H W - 1) is a multiple of 8


def draw_case(rng, case):
    """One configuration.  The kind cycles with case % 10 (KINDS), the normalisation with case % 3: a spilled bucket in a batch of
    two, a short last strip with events on its seams, a sensor wider than 9600, integer coordinates and channel times (tied
    thresholds), a sparse window clipped at 0.1 (zero threshold), an integer quantile rank, times outside [first, last] and
    unsorted, two free draws, and a ragged batch with an empty sample."""
    kind = KINDS[case % 10]
    c = {'case': case, 'kind': kind, 'norm': (None, 'mean_std', 'max')[case % 3], 'B': rng.choice([1, 1, 2, 3]),
         'q': rng.choice([0.0, 0.0, 0.02, 0.05, 0.1, 0.125]), 'seed': rng.randrange(1 << 30)}
    if kind == 'spill':
        c.update(shape=(rng.choice([3, 4, 5]), 10, 2400), n=rng.randrange(4400, 6000), B=2, q=rng.choice([0.0, 0.0, 0.05]))
    elif kind == 'short':
        H, W = rng.choice(SHORT_HW)
        c.update(shape=(rng.choice([1, 2, 3]), H, W), n=rng.randrange(500, 3000))
    elif kind == 'wide':
        c.update(shape=(rng.choice([1, 2]), rng.choice([1, 2, 3]), rng.randrange(9601, 12001)), n=rng.randrange(200, 3000))
    elif kind == 'integer':
        shape = (rng.choice([2, 3, 5]), rng.randrange(4, 25), rng.randrange(4, 33))
        c.update(shape=shape, n=int(shape[0] * shape[1] * shape[2] * rng.uniform(0.6, 1.0)), q=rng.choice([0.02, 0.05, 0.1]))
    elif kind == 'sparse':
        shape = (rng.choice([3, 5]), rng.randrange(16, 25), rng.randrange(20, 33))
        c.update(shape=shape, n=max(2, shape[0] * shape[1] * shape[2] // 100), q=0.1, B=rng.choice([1, 2]))
    elif kind == 'intrank':
        c.update(shape=rng.choice(INTRANK_SHAPES), n=rng.randrange(2, 300), q=0.125)
    else:
        c.update(shape=(rng.choice([1, 2, 3, 5, 15]), rng.randrange(1, 40), rng.randrange(1, 60)), n=rng.randrange(2, 3000))
        if kind == 'ragged':
            c['B'] = 3
    return c


def tag_of(c):
    return ' '.join(f'{k}={v}' for k, v in c.items())


def make_case(c):
    import voxel_cases as VC
    shape, n, kind = c['shape'], c['n'], c['kind']
    C, H, W = shape
    samples = []
    for b in range(c['B']):
        g = VC.gen(c['seed'] + 7919 * b)
        nb = n if b == 0 else max(2, int(n * float(torch.rand(1, generator=g))))
        if kind == 'ragged' and b == 1:
            samples.append(tuple(torch.zeros(0) for _ in range(4)))
            continue
        x, y, t, p = VC.uniform_events(nb, shape, g)
        if kind == 'spill':                     # one strip (rows 4..7) and one pair of channels: more records than a bucket holds
            y = VC.coords(nb, 4, 7, g)
            t = torch.sort((1.0 + VC.frac(nb, g)) / (C - 1)).values
            t[0], t[-1] = 0.0, 1.0
        elif kind == 'short':                   # a third of the events on the seams between the strips
            SR = VC.vox_geometry(shape, n, c['B'])['SR']
            k = nb // 3
            y[:k] = (SR * torch.randint(1, -(-H // SR), (k,), generator=g) - 1).float() + VC.frac(k, g)
        elif kind == 'integer':
            x, y = torch.randint(0, W, (nb,), generator=g).float(), torch.randint(0, H, (nb,), generator=g).float()
            t = torch.sort(torch.randint(0, C, (nb,), generator=g).float() / (C - 1)).values
            t[0], t[-1] = 0.0, 1.0
        elif kind == 'time' and nb > 2:         # t_norm from -2 to C + 1, shuffled, the first and last rows pinned
            tn = torch.randint(-2, C + 1, (nb,), generator=g).float() + VC.frac(nb, g)
            t = 0.25 + 0.5 * tn / max(C - 1, 1)
            t[0], t[-1] = 0.25, 0.75
        samples.append((x, y, t, p))
    N = max(s[0].numel() for s in samples) + (5 if kind == 'ragged' else 0)
    return VC.Case(f'fuzz{c["case"]}', shape, samples, ((c['norm'], c['q']),), N=N)


def run_case(c, dev, stats):
    """-> list of failure strings (empty: the case passes), or None: the inputs break a cap and the case is to be redrawn."""
    import voxel_cases as VC
    from motionpriorcmax_amd.utils import voxel_grids
    case = make_case(c)
    norm, q = c['norm'], c['q']
    exp = [VC.oracles(ev, case.shape, norm, q) for ev in case.expect]
    if any(VC.input_caps(o) != (0, 0) for o in exp):
        return None
    geo = case.geometry()
    C, H, W = case.shape
    took = dict.fromkeys(ROUTES, False)
    took['NS > 1'] = geo['NS'] > 1
    took['short last strip'] = H < geo['NS'] * geo['SR']
    took['spill'] = any(int(case.fills(b).max()) > geo['cap'] for b in range(case.B))
    took['B > 1'] = case.B > 1
    took['empty sample'] = any(n == 0 for n in case.counts)
    took['q > 0'] = q > 0
    took['wide sensor'] = VC.VOX_STRIP_KB * 1024 // (W * 8) == 0
    for (x, y, t, p), o in zip(case.samples, exp):
        if t.numel() and (bool((t < t[0]).any()) or bool((t > t[-1]).any())):
            took['times outside [first, last]'] = True
        if t.numel() > 2 and bool((x == x.floor()).all()) and bool((y == y.floor()).all()):
            took['integer coordinates'] = True
        if q > 0 and bool(o['raw64'].any()):
            below, k0, k1, tied = VC.threshold_info(o['raw64'], q)
            took['zero threshold'] |= below == 0 and (tied or k1 == k0)
            took['tied threshold'] |= tied and below > 0
            took['integer rank'] |= k1 == k0
    for r, t in took.items():
        stats['routes'][r] += int(bool(t))
    ev, cnt = case.batch()
    out = voxel_grids(ev.to(dev), cnt.to(dev), case.shape, norm, q).cpu()
    fails = []
    for b, o in enumerate(exp):
        d = float((out[b].double() - o['g64']).abs().max())
        bound = VC.bound_of(o)[0]
        ratio = d / bound if bound > 0 else (0.0 if d == 0 else float('inf'))
        stats['worst'] = max(stats['worst'], ratio)
        if not bool(torch.isfinite(out[b]).all()):
            fails.append(f'sample {b}: non-finite entries')
        elif not ratio <= 1.0:
            fails.append(f'sample {b}: |gpu - f64| {d:.3e} is {ratio:.2f} of the bound {bound:.3e}')
        nzz = int(((o['g64'] == 0) & (out[b] != 0)).sum())
        if nzz:
            fails.append(f'sample {b}: {nzz} entries are zero in float64 and not on the device')
    return fails


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    dev = torch.device('cuda:0')
    stats = {'routes': {r: 0 for r in ROUTES}, 'worst': 0.0}
    bad = redrawn = 0
    t0 = time.perf_counter()
    for case in range(n_cases):
        c = draw_case(rng, case)
        fails = None
        for _ in range(4):
            tag = 'case ' + tag_of(c)
            if os.environ.get('FUZZ_VERBOSE'):
                print(tag, flush=True)
            try:
                fails = run_case(c, dev, stats)
            except Exception as e:      # noqa: BLE001 -- report and go on, unless the device itself failed
                fails = ['ERROR ' + repr(e)[:300]]
                if any(w in repr(e) for w in ('HIP error', 'hipError', 'CUDA error', 'illegal memory access', 'rc=700', 'rc=719')):
                    # (a fault of the device: nothing more is started on it; the cases not run count as bad)
                    print('MISMATCH', tag, '|', fails[0], '| DEVICE FAULT: stopping,', n_cases - case - 1, 'cases not run', flush=True)
                    print(f'{n_cases} cases, {bad + n_cases - case} bad')
                    sys.exit(1)
            if fails is not None:
                break
            redrawn += 1
            c['seed'] = rng.randrange(1 << 30)
        if fails is None:
            fails = ['the inputs broke a cap in four draws']
        if fails:
            bad += 1
            print('MISMATCH', tag, '|', ' ; '.join(fails), flush=True)
    torch.cuda.synchronize()
    print('routes: ' + ', '.join(f'{r}: {n}' for r, n in stats['routes'].items()))
    print(f'worst ratio to the bound {stats["worst"]:.3f}; {redrawn} cases redrawn; {time.perf_counter() - t0:.1f} s for the cases (oracle included)')
    if 10 * redrawn > n_cases:
        bad += 1
        print('TOO MANY REDRAWN')
    if n_cases >= 30:
        for r, n in stats['routes'].items():
            if n == 0:
                bad += 1
                print('UNCOVERED', r)
    print(f'{n_cases} cases, {bad} bad')
    from motionpriorcmax_amd import _lib as _C
    _n = _C.lib().mpc_bounds_check()
    print('mpc_bounds_check:', _n, _C.lib().mpc_last_error_string().decode() if _n > 0 else '')


if __name__ == '__main__':
    main()
