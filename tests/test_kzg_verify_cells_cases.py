"""The case builders of the cell verifier's tests check themselves in Python integers (no library involved): the interpolation polynomial of a cell goes through the cell's
values on the cell's coset, and a blob's polynomial minus it is the proof's quotient times the coset's vanishing polynomial -- the identity the pairing equation states at tau."""
import random
import pytest
from kzg_cases import R, horner
from kzg_cells_cases import to_coeffs, cells, cell_points, cell_shift, cell_quotient
from kzg_verify_cells_cases import interp_coeffs, neg_rows, neg_sums, cells_per_blob

SHAPES = [(1, 0), (1, 1), (2, 1), (5, 5), (6, 0), (8, 3), (7, 6)]


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_interpolation_goes_through_the_cell(log2_n, log2_cell):
    rnd = random.Random(7000 + 16 * log2_n + log2_cell)
    f = [rnd.randrange(R) for _ in range(1 << log2_n)]
    cs, m = cells(f, log2_n, log2_cell), cells_per_blob(log2_n, log2_cell)
    for k in sorted({0, 1, m // 2, m - 1}):
        a = interp_coeffs(cs[k], k, log2_n, log2_cell)
        assert len(a) == 1 << log2_cell
        assert [horner(a, x) for x in cell_points(k, log2_n, log2_cell)] == cs[k], k


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_polynomial_minus_interpolation_is_quotient_times_vanishing(log2_n, log2_cell):
    rnd = random.Random(7100 + 16 * log2_n + log2_cell)
    n, c = 1 << log2_n, 1 << log2_cell
    f = [rnd.randrange(R) for _ in range(n)]
    coef, cs, m = to_coeffs(f, log2_n), cells(f, log2_n, log2_cell), cells_per_blob(log2_n, log2_cell)
    for k in sorted({0, 1, m // 2, m - 1}):
        a, q, s = interp_coeffs(cs[k], k, log2_n, log2_cell), cell_quotient(coef, k, log2_n, log2_cell), pow(cell_shift(k, log2_n, log2_cell), c, R)
        prod = [0] * (n + c)          # q (X^c - s)
        for i, qi in enumerate(q):
            prod[i + c] = (prod[i + c] + qi) % R
            prod[i] = (prod[i] - s * qi) % R
        assert not any(prod[n:])
        assert prod[:n] == [(p - (a[i] if i < c else 0)) % R for i, p in enumerate(coef)], k
        for x in (rnd.randrange(R), 0, 1):          # and at points: the equation the pairing checks at tau
            assert (horner(coef, x) - horner(a, x)) % R == horner(q, x) * (pow(x, c, R) - s) % R


def test_rows_and_sums_agree():
    rnd = random.Random(7200)
    log2_n, log2_cell = 5, 2
    f = [rnd.randrange(R) for _ in range(32)]
    cs = cells(f, log2_n, log2_cell)
    idx = [3, 0, 15, 3]
    picked, w = [cs[k] for k in idx], [1 << 63, (1 << 64) - 1, 5, 0]
    rows = neg_rows(picked, idx, log2_n, log2_cell, out={2})
    assert rows[2] == [0] * 4 and rows[0] == rows[3]
    want = [sum(wk * r[i] for wk, r in zip(w, rows)) % R for i in range(4)]
    assert neg_sums(picked, idx, w, log2_n, log2_cell, out={2}) == want
