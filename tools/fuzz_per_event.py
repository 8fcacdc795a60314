"""Randomised differential test of the per-event basis warp (`FocusLoss.calc_per_event_basis`: k_pe_warp / k_pe_grad / k_pe_accum,
k_tile_rows[_bwd], k_basis_field, k_rows_grad_finish, mpc_event_pos_grad) against its DEFINITION on the CPU
(`oracle.focus_oracle.FocusLossOracle.calc_per_event_basis`) over random small configurations: superpixel, image shapes that are
no multiple of it (tiles without a centre included), scales, batch, bins (> 64 too), event counts, empty polarity blocks, padding,
basis and orders, the three backward variants, flags, objective, smoothness, t_ref (float / device tensor, 0 and 1), a scaled
backward (loss * c), event placement (uniform / one LUT row / a 3 x 3 spot).  Diagnostics; run on a GPU box:

    python tools/fuzz_per_event.py [n_cases] [seed]

Per case: loss at 1e-5 of the oracle's, IWEs at 1e-5 of their maximum, the gradient through grad_accounting.per_event_accounting;
for sign-free objectives ('l2' / variance) also relative L2 < 1e-4 -- where the fp32 oracle itself misses that against the same
oracle in float64 (few events), the case is judged against float64 at 4 times the fp32 oracle's own distance, both figures
printed; a case past one of the accounting's caps (fractions of the tile count) is judged against float64 by the same
rule; exact zeros off the tile centres and over tiles without a centre; ordered cases run twice, bitwise equal (the gradient
only where the LDS backward ran).  The rare branches are a fixed share of the cases (see `draw_case`), and the summary counts the
routes taken: with 30 cases or more, a route that no case took counts as bad.

Measured on an MI355X with `30 24` (0 bad; every route taken: k_pe_accum 4, k_pe_grad with an ordered batch 5, k_pe_grad unordered 9,
torch cross-check 9, S > 1 21, non-divisible 20, missing tile centre 14, nb > 64 7, empty polarity block 8, grad_out != 1 14):
worst loss difference 0.024 of its bound; worst |gradient difference| / max |gradient|: fused atomics 7.2e-6, ordered LDS 1.8e-6,
torch 1.2e-3, ordered batch on atomics 1.1 (explained sign flips of an 'l1' case); sign-free relative L2 at most 0.026 of 1e-4 (the
float64 rule was never needed there); one case (10: 'l1', 425 tiles, 66 % of them explained) is past an accounting cap and judged
against float64 (device 7.1e-7, fp32 oracle 7.2e-7 from it: 0.007 of the rule); 1.6 s for the 30 cases, oracle included (3.2 s as a test, with the process start).
With the kernels broken on purpose (each in a build of its own): without the scale loop of k_tile_rows 5 of the 30 cases are bad
(4, 7, 9, 22, 27), without `* go` in k_rows_grad_finish 2 (0, 28); `j / SPLIT == part` for `j % SPLIT == part` in k_pe_accum passes
all 30 -- at these image sizes split is 16 and part 0 then takes every range; tests/test_gpu_per_event.py's split = 1 test catches it.
The small-weight ratio of that file: 0.705 of the bound (1.276 with the truncating conversion k_pe_accum had before).

`python tools/fuzz_per_event.py table [n_cases] [seed]`: the same configurations with a TABULATED basis (basis_type='table': random
samples S -- 1, a few, 1024, past the library's limit --, k, t_ref, flags) against tests/pe_table_cases.py's definition: loss and
IWEs as above; the coefficient AND the table gradient by relative L2 (1e-4 sign-free, 2e-3 'l1') or, past that, against float64 at
4 times the fp32 definition's own distance; ordered cases twice, the table gradient bitwise equal.
Measured on an MI355X with `table 150 7`, product and -DMPC_BOUNDS build alike: 0 bad, mpc_bounds_check 0; routes k_pe_table_grad 41,
k_pe_accum 17, k_pe_grad 24, k_field_basis_grad_part 28, plain torch 72; worst loss ratio 0.049, worst relative L2 / bound: coefficients
0.037, table 0.766; four cases judged against float64 (worst 0.007 of that rule); 2.2 s (profiles/pe_table_bounds_run.txt).
"""
import math
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))          # grad_accounting: the accountable gradient check the suite uses
import numpy as np
import torch

ROUTES = ('k_pe_accum', 'k_pe_grad ordered batch', 'k_pe_grad unordered', 'torch cross-check', 'S > 1', 'non-divisible shape',
          'missing tile centre', 'nb > 64', 'empty polarity block', 'grad_out != 1')


def centres(n, sp):
    """Tile centres sp // 2, sp // 2 + sp, ... inside [0, n)."""
    return len(range(sp // 2, n, sp))


def draw_case(rng, case):
    """One configuration.  The rare branches come round by the case index, not by luck: the variant cycles with case % 3; cases
    0, 1 of every 15 are 'big' (sp = 2 near 96 x 128 with k >= 8: a LUT strip's accumulators pass the LDS limit, an ordered batch
    falls back to k_pe_grad); case % 10 == 3 has 65 bins; case % 4 == 2 has a tile without a centre."""
    c = {'case': case}
    c['variant'] = ('ordered', True, False)[case % 3]
    big = case % 15 in (0, 1)
    sp = 2 if big else rng.choice([2, 3, 4, 8])
    lo_h, hi_h, lo_w, hi_w = (90, 100, 120, 140) if big else (8, 100, 8, 140)

    def side(lo, hi, rem):
        """A multiple of sp in [lo, hi], plus a remainder: '' none, 'lost' 1..sp // 2 (the last cell has no centre), 'any' 1..sp - 1."""
        n = sp * rng.randrange(-(-lo // sp), hi // sp + 1)
        if rem:
            r = rng.randrange(1, (sp // 2 if rem == 'lost' else sp - 1) + 1)
            n = n + r if n + r <= hi else n - sp + r
        return n
    # about half the cases are no multiple of sp (on one side or both); every fourth case loses a tile centre for certain
    rem = 'lost' if case % 4 == 2 else rng.choice(['', '', 'any', 'any'])
    sides = rng.choice(['h', 'w', 'hw'])
    c['sp'], c['H'], c['W'] = sp, side(lo_h, hi_h, rem if 'h' in sides else ''), side(lo_w, hi_w, rem if 'w' in sides else '')
    c['S'] = rng.choice([1, 2, 3])
    c['B'] = rng.choice([1, 2, 3])
    c['nb'] = 65 if case % 10 == 3 else rng.choice([1, 2, 5, 15]) if big else rng.choice([1, 2, 5, 15, 65])
    c['M'] = rng.choice([0, 1, 50, 2000, 2000, 12000, 12000])
    c['num_pos'] = rng.choice(['balanced', 0, 'M'])
    c['pad_frac'] = rng.choice([0.0, 0.1])
    c['all_pad_sample'] = rng.random() < 0.2
    c['k'] = rng.choice([8, 9, 12]) if big else rng.choice([1, 2, 3, 4, 8, 9, 12])
    c['basis'] = rng.choice(['polynomial', 'dct'])
    c['scale_iwe_by_dt'], c['mask_image_border'] = rng.random() < 0.5, rng.random() < 0.5
    c['polarity_aware_batching'] = rng.random() < 0.6
    c['focus_loss_norm'] = rng.choice(['l1', 'l2'])
    c['loss_type'] = rng.choice(['gradient_magnitude', 'variance'])
    c['smooth_weight'] = rng.choice([0.0, 0.003, 0.06])
    c['t_ref'] = rng.choice([0.0, 1.0, rng.random()])
    c['t_ref_as'] = rng.choice(['float', 'tensor'])
    c['gscale'] = rng.choice([1.0, -2.5])
    c['placement'] = rng.choice(['uniform', 'uniform', 'band', 'spot'])
    c['sigma'] = rng.choice([0.5, 4.0, 4.0])           # (4: some events leave the image)
    c['seed'] = rng.randrange(1 << 30)
    return c


def tag_of(c):
    return ' '.join(f'{k}={v}' for k, v in c.items())


def make_inputs(c):
    from oracle import focus_oracle as O
    H, W, sp, B, M, nb, k = c['H'], c['W'], c['sp'], c['B'], c['M'], c['nb'], c['k']
    g = torch.Generator().manual_seed(c['seed'])
    num_pos = {'balanced': None, 0: 0, 'M': M}[c['num_pos']]
    ev, num_pos = O.synth_events(B, M, (H, W), nb, seed=c['seed'], pad_frac=c['pad_frac'], num_pos=num_pos)
    rows = ev[..., 5] > 0
    # positions over the whole image, [0, H) x [0, W): the last cells (with or without a centre) get their events
    y, x = torch.rand(B, M, generator=g) * H, torch.rand(B, M, generator=g) * W
    if c['placement'] != 'uniform':
        hq = -(-H // sp)
        r = int(torch.randint(0, hq, (1,), generator=g))
        y = torch.rand(B, M, generator=g) * (min(r * sp + sp, H) - r * sp) * 0.999 + r * sp          # one LUT row high: one strip
        if c['placement'] == 'spot':
            y0, x0 = float(torch.rand(1, generator=g)) * max(H - 3, 0), float(torch.rand(1, generator=g)) * max(W - 3, 0)
            y, x = y0 + torch.rand(B, M, generator=g) * 3, x0 + torch.rand(B, M, generator=g) * 3
    ev[..., 0], ev[..., 1] = torch.where(rows, y, ev[..., 0]), torch.where(rows, x, ev[..., 1])
    if c['all_pad_sample'] and M > 0:
        ev[int(torch.randint(0, B, (1,), generator=g))] = 0
    coeff = torch.randn(B, c['S'], 2 * k, H, W, generator=g) * c['sigma']
    t_ref = float(np.float32(c['t_ref']))                # (the value the device works with)
    cfg = dict(image_shape=(H, W), num_tref=1, num_bins=nb, num_knn=1, smooth_weight=c['smooth_weight'], lut_superpixel_size=sp,
               focus_loss_norm=c['focus_loss_norm'], dist_norm='l2', scale_iwe_by_dt=c['scale_iwe_by_dt'],
               mask_image_border=c['mask_image_border'], polarity_aware_batching=c['polarity_aware_batching'],
               interpolation_scheme='mean', smooth_type='on_flow_to_tref', loss_type=c['loss_type'])
    return cfg, ev, num_pos, coeff, t_ref


def oracle_run(cfg, ev, num_pos, coeff, t_ref, k, basis, gscale, dtype=torch.float32):
    from oracle import focus_oracle as O
    co = coeff.to(dtype).clone().requires_grad_(True)
    lo, _, mo = O.FocusLossOracle(**cfg).calc_per_event_basis(co, t_ref, {'events': ev.to(dtype), 'num_pos_events': num_pos}, k, basis)
    if torch.isfinite(lo):
        (lo * gscale).backward()
    return float(lo.detach()), mo['iwes'], (co.grad if co.grad is not None else torch.zeros_like(co)).detach()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def run_case(c, dev, stats):
    """-> list of failure strings (empty: the case passes)."""
    from motionpriorcmax_amd import LossFactory, ops
    from grad_accounting import per_event_accounting
    from oracle import focus_oracle as O
    cfg, ev, num_pos, coeff, t_ref = make_inputs(c)
    H, W, sp, k, basis, variant, gscale = c['H'], c['W'], c['sp'], c['k'], c['basis'], c['variant'], c['gscale']
    hq, wq, hc, wc = -(-H // sp), -(-W // sp), centres(H, sp), centres(W, sp)
    lo, iwo, go = oracle_run(cfg, ev, num_pos, coeff, t_ref, k, basis, gscale)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if variant == 'ordered':
        batch = L.order_events(batch)
    t_dev = t_ref if c['t_ref_as'] == 'float' else torch.tensor(t_ref, device=dev)

    def device_run():
        cg = coeff.to(dev).requires_grad_(True)
        lg, _, mg = L.calc_per_event_basis(cg, t_dev, batch, k, basis, fused=bool(variant))
        if bool(torch.isfinite(lg)):
            (lg * gscale).backward()
        return lg.detach(), mg['iwes'], (cg.grad if cg.grad is not None else torch.zeros_like(cg)).detach()
    with ops.KernelTimer() as kt:
        lg, iwg, gg = device_run()
    ran = kt.summary()
    fails = []
    lg_v = float(lg)
    finite = math.isfinite(lo)
    # routes
    accum, atomic = 'k_pe_accum' in ran, 'k_pe_grad' in ran
    took = {'k_pe_accum': accum, 'k_pe_grad ordered batch': atomic and variant == 'ordered', 'k_pe_grad unordered': atomic and variant is True,
            'torch cross-check': variant is False and finite, 'S > 1': c['S'] > 1, 'non-divisible shape': H % sp != 0 or W % sp != 0,
            'missing tile centre': (hc, wc) != (hq, wq), 'nb > 64': c['nb'] > 64,
            'empty polarity block': cfg['polarity_aware_batching'] and num_pos in (0, c['M']), 'grad_out != 1': gscale != 1.0 and finite}
    for r, t in took.items():
        stats['routes'][r] += int(bool(t))
    if not finite:
        if math.isfinite(lg_v):
            fails.append(f'the oracle loss is {lo}, the device loss {lg_v}')
        return fails
    # loss and IWEs
    lr = abs(lg_v - lo) / (1e-5 * abs(lo))
    stats['loss'] = max(stats['loss'], lr)
    if not lr <= 1.0:
        fails.append(f'loss {lg_v!r} against {lo!r}: {lr:.2f} of the bound')
    iw = iwo.reshape(iwg.shape)
    if not float((iwg.cpu() - iw).abs().max()) <= 1e-5 * float(iw.abs().max()):
        fails.append(f'IWE differs by {float((iwg.cpu() - iw).abs().max()):.3e}, max {float(iw.abs().max()):.3e}')
    # gradient
    g = gg.cpu()
    vname = {True: 'fused atomics', False: 'torch', 'ordered': 'ordered LDS' if accum else 'ordered -> atomics'}[variant]
    if not bool(torch.isfinite(g).all()):
        fails.append('non-finite gradient')
        return fails
    m = O.tile_mask((H, W), sp)
    if float(g[..., ~m].abs().max()) != 0.0:
        fails.append('gradient off the tile centres')
    if hc < hq and float(g[..., (hq - 1) * sp:, :].abs().max()) != 0.0 or wc < wq and float(g[..., (wq - 1) * sp:].abs().max()) != 0.0:
        fails.append('gradient over a tile without a centre')
    if float(go.abs().max()) == 0.0:
        # (no event votes with a gradient and no smoothness term: every product the kernels add is an exact zero)
        if float(g.abs().max()) != 0.0:
            fails.append(f'the oracle gradient is zero, the device gradient up to {float(g.abs().max()):.3e}')
    else:
        # Every mismatch must be explained, in every case (asserted inside).  The accounting's two caps -- at most 1 % of the tiles
        # mismatch, the excuse covers at most 25 % of them -- are fractions of the tile count; an image here has as few as one
        # tile.  A case that passes a cap is not let through on that: it is judged against the float64 oracle instead, at 4 times
        # the fp32 oracle's own distance from it (the project's relative L2 bound 1e-4 as the floor), and is bad if it misses.
        capped = False
        try:
            res = per_event_accounting(cfg, ev, num_pos, coeff, t_ref, k, basis, g, go, label=f'case {c["case"]}', caps=False)
            stats['grad'][vname] = max(stats['grad'].get(vname, 0.0), res['worst'])
            capped = not res['caps_hold']
        except AssertionError as e:
            fails.append('accounting: ' + str(e)[:300])
        if capped:
            stats['capped'] += 1
            _, _, g64 = oracle_run(cfg, ev, num_pos, coeff, t_ref, k, basis, gscale, torch.float64)
            d_or, d_dev = rel_l2(go, g64), rel_l2(g, g64)
            print(f'case {c["case"]}: past an accounting cap (mismatching {100 * res["frac_mismatch_origin"]:.2f} %, explained '
                  f'{100 * res["frac_excuse"]:.2f} % of the tiles); against float64: fp32 oracle {d_or:.3e}, device {d_dev:.3e}', flush=True)
            if not d_dev <= max(4 * d_or, 1e-4):
                fails.append(f'past an accounting cap, and relative L2 to float64 {d_dev:.3e} > 4 x {d_or:.3e} (the fp32 oracle)')
            else:
                stats['cap_64'] = max(stats['cap_64'], d_dev / max(4 * d_or, 1e-4))
        if cfg['focus_loss_norm'] == 'l2' or cfg['loss_type'] == 'variance':
            r32 = rel_l2(g, go)
            if r32 < 1e-4:
                stats['l2'][vname] = max(stats['l2'].get(vname, 0.0), r32 / 1e-4)
            else:
                _, _, g64 = oracle_run(cfg, ev, num_pos, coeff, t_ref, k, basis, gscale, torch.float64)
                d_or, d_dev = rel_l2(go, g64), rel_l2(g, g64)
                print(f'case {c["case"]}: relative L2 to the fp32 oracle {r32:.3e} >= 1e-4; against float64: fp32 oracle {d_or:.3e}, device {d_dev:.3e}', flush=True)
                if d_or < 1e-4:
                    fails.append(f'relative L2 {r32:.3e} of the gradient (the fp32 oracle is {d_or:.3e} from float64)')
                elif not d_dev <= 4 * d_or:
                    fails.append(f'relative L2 to float64 {d_dev:.3e} > 4 x {d_or:.3e} (the fp32 oracle)')
                else:
                    stats['l2_64'] = max(stats['l2_64'], d_dev / (4 * d_or))
    if variant == 'ordered':
        l2, _, g2 = device_run()
        if not torch.equal(l2, lg):
            fails.append(f'ordered batch: the loss of a second run differs ({float(l2)!r}, {lg_v!r})')
        if accum and not atomic and not torch.equal(g2, gg):
            fails.append('ordered batch (LDS backward): the gradient of a second run differs')
    return fails


def run_table_case(c, dev, stats):
    """The `table` mode: -> list of failure strings."""
    from motionpriorcmax_amd import LossFactory, ops
    import pe_table_cases as PT
    cfg, ev, num_pos, coeff, t_ref = make_inputs(c)
    k, variant, gscale, S = c['k'], c['variant'], c['gscale'], c['samples']
    g = torch.Generator().manual_seed(c['seed'] + 1)
    table = torch.randn(S + 1, k, generator=g) * 0.5 if S <= 2048 else torch.cumsum(torch.randn(S + 1, k, generator=g) * 0.02, 0)

    def definition(dtype):
        co, tb = coeff.to(dtype).clone().requires_grad_(True), table.to(dtype).clone().requires_grad_(True)
        lo, iw = PT.calc_per_event_table(cfg, co, tb, t_ref, {'events': ev.to(dtype), 'num_pos_events': num_pos})
        if torch.isfinite(lo):
            (lo * gscale).backward()
        z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach()
        return float(lo.detach()), iw, z(co), z(tb)
    lo, iwo, gco, gto = definition(torch.float32)
    L = LossFactory.get_loss_calculator('FOCUS', cfg)
    batch = {'events': ev.to(dev), 'num_pos_events': num_pos}
    if variant == 'ordered':
        batch = L.order_events(batch)
    t_dev = t_ref if c['t_ref_as'] == 'float' else torch.tensor(t_ref, device=dev)

    def device_run():
        cg, tb = coeff.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
        lg, _, mg = L.calc_per_event_basis(cg, t_dev, batch, k, 'table', fused=bool(variant), basis_table=tb)
        if bool(torch.isfinite(lg)):
            (lg * gscale).backward()
        z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach()
        return lg.detach(), mg['iwes'], z(cg), z(tb)
    with ops.KernelTimer() as kt:
        lg, iwg, gc, gt = device_run()
    ran = kt.summary()
    for r in ('k_pe_table_grad', 'k_pe_accum', 'k_pe_grad', 'k_field_basis_grad_part'):
        stats['routes'][r] = stats['routes'].get(r, 0) + int(r in ran)
    stats['routes']['plain torch'] = stats['routes'].get('plain torch', 0) + int('k_pe_warp' not in ran and c['M'] * c['B'] > 0)
    fails = []
    if not math.isfinite(lo):
        if math.isfinite(float(lg)):
            fails.append(f'the definition\'s loss is {lo}, the device loss {float(lg)}')
        return fails
    lr = abs(float(lg) - lo) / (1e-5 * abs(lo))
    stats['loss'] = max(stats['loss'], lr)
    if not lr <= 1.0:
        fails.append(f'loss {float(lg)!r} against {lo!r}: {lr:.2f} of the bound')
    iw = iwo.reshape(iwg.shape)
    if not float((iwg.cpu() - iw).abs().max()) <= 1e-5 * float(iw.abs().max()):
        fails.append(f'IWE differs by {float((iwg.cpu() - iw).abs().max()):.3e}, max {float(iw.abs().max()):.3e}')
    bound = 1e-4 if (cfg['focus_loss_norm'] == 'l2' or cfg['loss_type'] == 'variance') else 2e-3
    g64 = None
    for what, gd, g32, idx in (('coefficient', gc.cpu(), gco, 2), ('table', gt.cpu(), gto, 3)):
        if not bool(torch.isfinite(gd).all()):
            fails.append(f'non-finite {what} gradient')
            continue
        if float(g32.abs().max()) == 0.0:
            if float(gd.abs().max()) != 0.0:
                fails.append(f'the definition\'s {what} gradient is zero, the device\'s up to {float(gd.abs().max()):.3e}')
            continue
        r32 = rel_l2(gd, g32)
        if r32 < bound:
            stats['l2'][what] = max(stats['l2'].get(what, 0.0), r32 / bound)
            continue
        g64 = g64 or definition(torch.float64)
        d_or, d_dev = rel_l2(g32, g64[idx]), rel_l2(gd, g64[idx])
        print(f'case {c["case"]}: {what} gradient: relative L2 to the fp32 definition {r32:.3e} >= {bound:.0e}; against float64: fp32 definition '
              f'{d_or:.3e}, device {d_dev:.3e}', flush=True)
        if d_or < bound:
            fails.append(f'relative L2 {r32:.3e} of the {what} gradient (the fp32 definition is {d_or:.3e} from float64)')
        elif not d_dev <= 4 * d_or:
            fails.append(f'{what} gradient: relative L2 to float64 {d_dev:.3e} > 4 x {d_or:.3e} (the fp32 definition)')
        else:
            stats['l2_64'] = max(stats['l2_64'], d_dev / (4 * d_or))
    if variant == 'ordered':
        l2, _, _, t2 = device_run()
        if not torch.equal(l2, lg):
            fails.append('ordered batch: the loss of a second run differs')
        if 'k_pe_table_grad' in ran and not torch.equal(t2, gt):
            fails.append('ordered batch: the table gradient of a second run differs')
    return fails


def main_table(argv):
    n_cases = int(argv[0]) if argv else 150
    rng = random.Random(int(argv[1]) if len(argv) > 1 else 0)
    dev = torch.device('cuda:0')
    from motionpriorcmax_amd import _lib as _C
    lim = int(_C.lib().mpc_pe_table_limit())
    stats = {'routes': {}, 'loss': 0.0, 'l2': {}, 'l2_64': 0.0}
    bad, t_dev = 0, 0.0
    for case in range(n_cases):
        c = draw_case(rng, case)
        c['basis'] = 'table'
        c['k'] = rng.choice([1, 2, 3, 4, 8, 9])
        c['samples'] = rng.choice([1, 1, 2, 7, 37, 256, 1024, 1024, lim // c['k'] - 1, lim // c['k']])
        c['M'] = min(c['M'], 2000) if c['samples'] > 2048 else c['M']
        tag = 'case ' + tag_of(c)
        try:
            t0 = time.perf_counter()
            fails = run_table_case(c, dev, stats)
            torch.cuda.synchronize()
            t_dev += time.perf_counter() - t0
        except Exception as e:      # noqa: BLE001
            fails = ['ERROR ' + repr(e)[:300]]
            if any(w in repr(e) for w in ('HIP error', 'hipError', 'CUDA error', 'illegal memory access', 'rc=700', 'rc=719')):
                bad += n_cases - case
                print('MISMATCH', tag, '|', fails[0], '| DEVICE FAULT: stopping,', n_cases - case - 1, 'cases not run', flush=True)
                break
        if fails:
            bad += 1
            print('MISMATCH', tag, '|', ' ; '.join(fails), flush=True)
    print('table mode routes: ' + ', '.join(f'{r}: {n}' for r, n in stats['routes'].items()))
    print(f'worst loss ratio to its bound {stats["loss"]:.3f}; worst relative L2 / bound ' + ', '.join(f'{v}: {x:.3f}' for v, x in sorted(stats['l2'].items()))
          + f'; worst ratio to the float64 rule {stats["l2_64"]:.3f}; {t_dev:.1f} s for the cases (definition included)')
    if n_cases >= 30:
        for r in ('k_pe_table_grad', 'k_pe_accum', 'k_pe_grad', 'k_field_basis_grad_part', 'plain torch'):
            if stats['routes'].get(r, 0) == 0:
                bad += 1
                print('UNCOVERED', r)
    print(f'{n_cases} table cases, {bad} bad')
    _n = _C.lib().mpc_bounds_check()
    print('mpc_bounds_check:', _n, _C.lib().mpc_last_error_string().decode() if _n > 0 else '')


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'table':
        return main_table(sys.argv[2:])
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    dev = torch.device('cuda:0')
    stats = {'routes': {r: 0 for r in ROUTES}, 'loss': 0.0, 'grad': {}, 'l2': {}, 'l2_64': 0.0, 'capped': 0, 'cap_64': 0.0}
    bad = 0
    t_dev = 0.0
    for case in range(n_cases):
        c = draw_case(rng, case)
        tag = 'case ' + tag_of(c)
        if os.environ.get('FUZZ_VERBOSE'):
            print(tag, flush=True)
        if os.environ.get('FUZZ_LIST') and str(case) not in os.environ['FUZZ_LIST'].split(','):
            continue
        try:
            t0 = time.perf_counter()
            fails = run_case(c, dev, stats)
            torch.cuda.synchronize()
            t_dev += time.perf_counter() - t0
        except Exception as e:      # noqa: BLE001 -- report and go on, unless the device itself failed
            fails = ['ERROR ' + repr(e)[:300]]
            if any(w in repr(e) for w in ('HIP error', 'hipError', 'CUDA error', 'illegal memory access', 'rc=700', 'rc=719')):
                # (a fault of the device: nothing more is started on it; the cases not run count as bad)
                bad += n_cases - case
                print('MISMATCH', tag, '|', fails[0], '| DEVICE FAULT: stopping,', n_cases - case - 1, 'cases not run', flush=True)
                break
        if fails:
            bad += 1
            print('MISMATCH', tag, '|', ' ; '.join(fails), flush=True)
    print('routes: ' + ', '.join(f'{r}: {n}' for r, n in stats['routes'].items()))
    print(f'worst loss ratio to its bound {stats["loss"]:.3f}; worst |gradient difference| / max|gradient| per variant '
          + ', '.join(f'{v}: {x:.2e}' for v, x in sorted(stats['grad'].items()))
          + '; worst relative L2 / 1e-4 (sign-free) ' + ', '.join(f'{v}: {x:.3f}' for v, x in sorted(stats['l2'].items()))
          + f'; worst ratio to the float64 rule {stats["l2_64"]:.3f}; {t_dev:.1f} s for the cases (oracle included); {stats["capped"]} cases past an accounting cap, judged against float64: worst ratio {stats["cap_64"]:.3f}')
    if n_cases >= 30 and not os.environ.get('FUZZ_LIST'):
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
