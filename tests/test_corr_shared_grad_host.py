"""`shared_grad=True` of utils.CorrLookup on the host: the keyword is accepted by the three constructors, CPU tensors take the mirror with
ordinary autograd (the flag has no effect there: the same bits), and the C header's MPC_CORR_F_GRAD_ACCUM is mirrored by _lib."""
import os
import re

import torch

from conftest import ROOT, load_golden
from test_corr_lookup_host import lookup_of


def _chain(lk, p0, times, gos):
    """Three chained lookups, p_{k+1} = p_k + 0.01 * out_k[:, :2d]; (grad p_0, grad levels)."""
    p = p0.clone().requires_grad_(True)
    d2 = p.shape[1]
    pk, loss = p, 0.0
    for go in gos:
        out = lk.lookup_bezier(pk, times)
        loss = loss + (out * go).sum()
        pk = pk + 0.01 * out[:, :d2]
    return torch.autograd.grad(loss, [p] + lk.levels)


def test_the_keyword_is_accepted_by_every_constructor():
    from motionpriorcmax_amd import utils

    class Data:
        def __init__(self, corr, tix):
            self.corr, self.target_indices = corr, torch.tensor(tix)

    class Block:
        pass

    g = load_golden('g16_corr_c')
    lk, p, times = lookup_of(g)
    nl = lk.num_levels_per_target
    want = lk.lookup_bezier(p, times)
    assert lk.shared_grad is False
    a = utils.CorrLookup(lk.levels, nl, radius=lk.radius, shared_grad=True)
    assert a.shared_grad is True and a._token is None              # (CPU levels: no gate)
    f1, f2 = torch.from_numpy(g['fmap1']).requires_grad_(True), torch.from_numpy(g['fmap2'])
    b = utils.CorrLookup.from_fmaps(f1, f2, nl, radius=lk.radius, shared_grad=True)
    assert b.shared_grad is True and b._token is None and b.levels[0].requires_grad
    block = Block()
    block._corr_pyramid = [Data(lv, t) for lv, t in zip(lk.levels, lk.target_indices)]
    block._radius = lk.radius
    c = utils.CorrLookup.from_block(block, nl, shared_grad=True)
    assert c.shared_grad is True and utils.CorrLookup.from_block(block, nl).shared_grad is False
    for other in (a, b, c):
        assert torch.equal(other.lookup_bezier(p, times), want)


def test_on_cpu_tensors_the_flag_has_no_effect():
    from motionpriorcmax_amd import utils
    g = load_golden('g16_corr_d')
    lk, p, times = lookup_of(g)
    gen = torch.Generator().manual_seed(19)
    gos = [torch.from_numpy(g['g'])] + [torch.randn(g['g'].shape, generator=gen) for _ in range(2)]
    shared = utils.CorrLookup(lk.levels, lk.num_levels_per_target, radius=lk.radius, shared_grad=True)
    want, got = _chain(lk, p, times, gos), _chain(shared, p, times, gos)
    assert len(want) == len(got) == 1 + len(lk.levels)
    for a, b in zip(want, got):
        assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_the_header_flag_is_mirrored():
    from motionpriorcmax_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mpcmax.h')).read(), flags=re.S)
    macros = {m: int(v) for m, v in re.findall(r'#define (MPC_CORR_[A-Z_]+) (\d+)', header)}
    assert macros['MPC_CORR_F_GRAD_ACCUM'] == _lib.CORR_F_GRAD_ACCUM
    assert macros['MPC_CORR_F_GRAD_ACCUM'] != macros['MPC_CORR_F_LANE_PER_QUERY']
    assert macros['MPC_CORR_F_GRAD_ACCUM'] & macros['MPC_CORR_F_LANE_PER_QUERY'] == 0        # (flags: distinct bits)
    assert _lib.lib().mpc_version() == 107
