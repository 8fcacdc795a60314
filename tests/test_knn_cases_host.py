"""CPU checks of tests/knn_cases.py: its reference, evaluated in float32, is the oracle bit for bit and reproduces the neighbour
sets of the goldens that store them; every query of every case tells its K-th neighbour from the (K + 1)-th by more than 20
allowances; a float32 stand-in of the whole operation passes every case under the comparator and eleven mutants of it fail, each
by the name of the assertion meant to catch it; the plans restated from the library agree with what the cases are written for."""
import numpy as np
import pytest
import torch

import knn_cases as KC
from conftest import GOLDEN_CASES, load_golden
from oracle import focus_oracle as O


def _float32_lut(c):
    """The reference's own sets with the values in float32 and the oracle's operations (mean / weights from the float32 distances)."""
    ref = KC.reference(c)
    lut, nxt = [], []
    for b in range(c.B):
        for t in range(c.nb):
            i = ref['idx'][b, t]
            g = (c.traj[b, :c.T].permute(1, 0, 2) - c.traj[b, c.T + t][:, None, :])[i]
            if c.iwd:
                w = 1 / (ref['dist'][b, t] + O.IWD_EPS)
                w = w / w.sum(1, keepdim=True)
                lut.append((w[..., None, None] * g).sum(1))
            else:
                lut.append(g.mean(1))
            if c.has_next and t < c.nb - 1:
                nxt.append((c.traj[b, c.T + t + 1] - c.traj[b, c.T + t])[i].mean(1))
    return torch.stack(lut).reshape(c.B, c.nb, c.hq, c.wq, c.T, 2), (torch.stack(nxt).reshape(c.B, c.nb - 1, c.hq, c.wq, 1, 2) if nxt else None)


@pytest.mark.parametrize('name', ['lattice_l1_iwd_next', 'band_translate40', 'T2_17x33'])
def test_reference_in_float32_is_the_oracle_bit_for_bit(name):
    c = KC.case(name)
    lut, nxt, idx = O.interpolate_flow(c.traj[:, :c.T], c.traj[:, c.T:], (c.H, c.W), c.sp, c.K, c.norm, c.scheme, c.want_next, return_idx=True)
    ref = KC.reference(c)
    assert torch.equal(idx, ref['idx'])                              # ordered lists: the oracle's stable sort of every distance row
    mine, mine_next = _float32_lut(c)
    assert torch.equal(lut, mine)
    if c.has_next:
        assert torch.equal(nxt, mine_next)
    # and the float64 values are that, less its rounding
    assert KC.compare(lut, ref['lut'], ref['lut_allow']).ratio <= 1.0


def test_reference_reproduces_the_goldens_neighbour_sets():
    seen = 0
    for name in GOLDEN_CASES:
        g = load_golden(name)
        if 'ind_k_sorted' not in g:
            continue
        cfg = g['cfg']
        T = cfg['num_tref']
        traj = O.trajectories_at(torch.from_numpy(g['coeff_grid']), torch.from_numpy(g['times']), O.tile_mask(cfg['image_shape'], int(g['patch'])),
                                 int(g['num_basis']), str(g['basis_type']))
        H, W = cfg['image_shape']
        c = KC.Case(name='golden', H=H, W=W, sp=cfg['lut_superpixel_size'], K=cfg['num_knn'], norm=cfg['dist_norm'],
                    scheme=cfg['interpolation_scheme'], want_next=False, T=T, traj=traj.float().contiguous())
        idx, _ = KC._select(c)
        got = np.sort(idx[..., :c.K].numpy(), -1)
        assert (got == g['ind_k_sorted'].reshape(got.shape)).all(), name
        seen += 1
    assert seen >= 1


@pytest.mark.parametrize('name', sorted(KC.CASES))
def test_every_query_tells_its_kth_neighbour_from_the_next(name):
    c = KC.case(name)
    s = KC.separation(c)
    print(f'{name}: smallest separation {s:.4g} allowances')
    assert s > KC.SEPARATION, (name, s)


@pytest.mark.parametrize('name', sorted(KC.CASES))
def test_stand_in_passes_every_case(name):
    c = KC.case(name)
    KC.check_all(c, 'stand-in', KC.standin(c))


@pytest.mark.parametrize('mutant', sorted(KC.MUTANTS))
def test_every_mutant_fails_by_the_name_of_its_assertion(mutant):
    what, name = KC.MUTANTS[mutant]
    c = KC.case(name)
    with pytest.raises(AssertionError, match=rf'\] {what}:') as e:
        KC.check_all(c, mutant, KC.standin(c, mutant))
    print(f'{mutant} on {name}: {e.value}')


def test_mutant_list_covers_what_the_comparator_asserts():
    assert len(KC.MUTANTS) >= 11
    assert {w for w, _ in KC.MUTANTS.values()} >= {'kth index', 'tie flag', 'normaliser', 'tile maximum', 'flow_lut', 'flow_next', 'grad_traj'}
    assert all(n in KC.CASES for _, n in KC.MUTANTS.values()) and all(n in KC.CASES for n in KC.FN_CASES)


def test_comparator_rejects_what_it_should():
    ref, allow = torch.tensor([[1.0, 0.0], [2.0, 0.0]]), torch.tensor([[1e-6, 0.0], [1e-6, 0.0]])
    assert KC.compare(ref, ref, allow).ratio == 0.0
    r = KC.compare(ref.double() + torch.tensor([[0.0, 0.0], [5e-7, 0.0]]), ref, allow)
    assert abs(r.ratio - 0.5) < 1e-3 and r.index == (1, 0)
    assert KC.compare(ref.double() + torch.tensor([[0.0, 1e-30], [0.0, 0.0]]).double(), ref, allow).ratio == float('inf')
    assert KC.compare(ref + torch.tensor([[float('nan'), 0.0], [0.0, 0.0]]), ref, allow).ratio == float('inf')


def test_cases_are_what_their_names_say():
    for name in ('strip_h127_w9', 'strip_h128_w9', 'strip_h129_w9', 'strip_h8_w8'):
        c = KC.case(name)
        assert KC.strip_usable(c) and c.wq >= 2 * KC.r_init(c) + 2 and (c.hq, c.wq) == tuple(int(v[1:]) for v in name.split('_')[1:])
    for name in ('tiny_1x1_n_eq_K', 'tiny_7x9', 'tiny_3x40', 'K_97', 'K_129_l1', 'T2_17x33', 'T2_17x33_iwd_l1', 'T3_15x17'):
        assert not KC.strip_usable(KC.case(name)), name
    assert KC.case('tiny_1x1_n_eq_K').n == KC.case('tiny_1x1_n_eq_K').K and KC.case('K_eq_n_12x12').n == 32
    assert [KC.sort_plan(KC.case(f'plan_{v}'))[0] for v in (1, 64, 100, 135)] == [8, 4, 2, 1]
    assert KC.sort_plan(KC.case('global_sort'))[1] and (KC.case('global_sort').hq, KC.case('global_sort').wq) == (186, 193)
    assert not any(KC.sort_plan(KC.case(n))[1] for n in KC.CASES if n != 'global_sort')
    # lattices: an excluded point at exactly the K-th distance in most queries; the points at exactly that distance (the shell) number
    # 2 with 'l2' on the 4 / 4 lattice, 3 at sp 2 and up to 8 with 'l1': both sides of the KS_LMAX keys a lane ranks in registers
    biggest = {}
    for name, lo in (('lattice_l2_mean', 4000), ('lattice_l1_mean', 4000), ('lattice_sp2_patch4', 10000), ('lattice_sp4_patch2', 4000)):
        c = KC.case(name)
        ref = KC.reference(c)
        assert int(ref['tie'].sum()) > lo, name
        shell = (KC.distances(c.queries(), c.traj[0, 1], c.norm) == ref['dk'][0, 0][:, None]).sum(1)
        biggest[name] = int(shell.max())
        assert int((shell > 1).sum()) > c.hq * c.wq // 2, name
    assert biggest['lattice_l2_mean'] <= KC.KS_LMAX < biggest['lattice_l1_mean'], biggest
    assert len(set(biggest.values())) >= 3, biggest
    assert int(KC.reference(KC.case('dup_one_spot'))['tie'].sum()) == 128
    # the pairs: two points on a query centre, ranked by index alone
    ref = KC.reference(KC.case('dup_pairs'))
    assert int(((ref['dist'][..., 0] == 0) & (ref['dist'][..., 1] == 0) & (ref['idx'][..., 0] < ref['idx'][..., 1])).sum()) >= 2 * 7
    # piles: exactly that many points in each of the three cells, in every bin
    for count in (6, 7, 16, 17, 128, 129):
        c = KC.case(f'pile_{count}')
        for t in range(c.nb):
            p = c.traj[0, 1 + t]
            for cy, cx in KC.CELLS.values():
                assert int(((KC.cell_of(p[:, 0], 4) == cy) & (KC.cell_of(p[:, 1], 4) == cx)).sum()) == count, (count, cy, cx)
    c = KC.case('margin_points')
    cy = KC.cell_of(c.traj[0, 1, :, 0], 4)
    # (-7.5 cells is y = -28.5, the first coordinate of cell -7: the edge between the margin ring and what is clamped into it)
    for v, k in ((-7, 24), (-8, 12), (c.hq + 6, 12), (c.hq + 7, 12), (c.hq + 8, 12)):
        assert int((cy == v).sum()) >= k, v
    assert int((c.traj[0, 1, :, 0] == -28.5).sum()) == 12
    c = KC.case('bin_outside')
    assert float(c.traj[0, 2, :, 1].min()) > c.W + 400
    # emptied bands: far queries by the hundred where the family empties a band, none where it only thins the points
    far = lambda n: int((KC.reference(KC.case(n))['dk'] > KC.far_limit(KC.case(n))).sum())          # noqa: E731
    assert far('band_translate40') > 300 and far('band_diverge-45') > 300 and far('band_both_sides') > 300 and far('band_diverge+45') == 0
    # 'iwd': no point nearer than the keep-off radius to a centre, but for the six planted pairs of iwd_near_centre
    for name in KC.CASES:
        c = KC.case(name)
        if c.iwd:
            d2 = KC.reference(c)['dist'][..., 0]
            lim = KC.IWD_KEEP_OFF ** 2 if c.norm == 'l2' else KC.IWD_KEEP_OFF
            assert int((d2 < lim).sum()) == (6 if name == 'iwd_near_centre' else 0), name


def test_cases_are_deterministic():
    for name in ('pile_17', 'band_diverge-45', 'iwd_near_centre'):
        fn, args = KC.CASES[name]
        assert torch.equal(fn(name, *args).traj, KC.case(name).traj)
