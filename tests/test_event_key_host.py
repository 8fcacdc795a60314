"""The strip of a LUT cell row as csrc/ev_key_device.h computes it -- (int)(((float)iy + 0.5f) * (1.f / (float)CSR)), no integer
division in the hot kernels -- restated in numpy float32 operation by operation and held against iy // CSR: for every CSR in
1 .. 4096 and every cell row below EV_KEY_EXACT_ROWS, the bound the header states and proves, and at the row where the header
says exactness ends.  Both figures are read from the header, so the comment there cannot drift from what is checked here.

Every row is covered without visiting every (CSR, row) pair one by one: the formula is non-decreasing in iy (int -> float below
2^24, + 0.5 and the product with a positive constant are monotone, and so is truncation), so it equals iy // CSR on all of strip k
= rows [k * CSR, (k + 1) * CSR) as soon as it gives k at both ends of the strip.  The ends of every strip below the bound are
checked for every CSR (about 2 * bound * ln 4096 evaluations); that the formula is monotone, and the argument with it, is checked
directly as well -- every row below the bound for the CSR of the first mismatch and a few others, and every CSR over the first
2^14 rows."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'motionpriorcmax_amd', 'csrc', 'ev_key_device.h')
F32 = np.float32


def strip_f32(iy, csr):
    """ev_strip(iy, ev_strip_inv(CSR)), one float32 rounding per operation as the device code has them (-ffp-contract=off)."""
    inv = F32(1.0) / F32(csr)                                  # ev_strip_inv: a correctly rounded division
    return ((np.asarray(iy).astype(F32) + F32(0.5)) * inv).astype(np.int32)          # (int) truncates; the values are >= 0


def _header_figures():
    src = open(HEADER).read()
    bound = re.search(r'#define EV_KEY_EXACT_ROWS \(1 << (\d+)\)', src)
    first = re.search(r'first row filed one strip too high is ([\d ]+) at CSR (\d+)', src)
    assert bound and first, 'ev_key_device.h no longer states its bound / the first mismatch'
    return 1 << int(bound.group(1)), int(first.group(1).replace(' ', '')), int(first.group(2))


def _first_mismatch_at_strip_ends(csr, lim):
    """First row below `lim` at an end of a strip where the formula leaves iy // CSR; None: none (then, the formula being
    monotone, no row below `lim` does)."""
    k = np.arange(0, (lim - 1) // csr + 1, dtype=np.int64)
    worst = None
    for rows in (k * csr, k * csr + csr - 1):
        keep = rows < lim
        bad = np.nonzero(strip_f32(rows[keep], csr) != k[keep])[0]
        if len(bad):
            worst = int(rows[keep][bad[0]]) if worst is None else min(worst, int(rows[keep][bad[0]]))
    return worst


def test_header_states_a_bound_the_format_can_hold():
    bound, first, first_csr = _header_figures()
    assert bound <= 1 << 23, 'iy + 0.5 is not a float32 beyond 2^23'
    assert bound <= first and 1 <= first_csr <= 4096


def test_strip_equals_integer_division_for_every_row_below_the_bound():
    bound, _, _ = _header_figures()
    for csr in range(1, 4097):
        assert _first_mismatch_at_strip_ends(csr, bound) is None, csr


def test_the_formula_is_monotone_row_by_row():
    """What the strip-end argument rests on, and the same comparison without it."""
    bound, _, first_csr = _header_figures()
    rows = np.arange(bound, dtype=np.int64)
    for csr in (1, 2, 3, 255, 1000, first_csr, 4096):
        got = strip_f32(rows, csr)
        assert np.array_equal(got, rows // csr), csr
        assert (np.diff(got) >= 0).all(), csr
    rows = np.arange(1 << 14, dtype=np.int64)
    for csr in range(1, 4097):
        assert np.array_equal(strip_f32(rows, csr), rows // csr), csr


def test_exactness_ends_where_the_header_says():
    """The first row that goes wrong for a CSR in 1 .. 4096 is the header's, one strip too high, and nothing goes wrong before
    it: the proven bound lies 0.2 % below."""
    bound, first, first_csr = _header_figures()
    assert int(strip_f32(first, first_csr)) == first // first_csr + 1
    assert int(strip_f32(first - 1, first_csr)) == (first - 1) // first_csr
    rows = np.arange(bound, first + 1, dtype=np.int64)          # the 7 166 rows between the bound and that row, one by one
    for csr in range(1, 4097):
        bad = rows[strip_f32(rows, csr) != rows // csr]
        assert bad.tolist() == ([first] if csr == first_csr else []), (csr, bad[:5])
