"""The Python side of the PeerDAS tests against itself (no library): the O(N log N) transform of kzg_cells_cases.py against Horner's rule, the identities the device code is
built on -- the extension as one coset evaluation, the points of a cell, the vanishing polynomial X^c - s_k -- and the recurrence of the quotient against long division."""
import random
import pytest
from kzg_cases import R, roots, horner, evals_of, eval_roots
from kzg_cells_cases import omega, to_evals, to_coeffs, coset_shift, cells, cell_shift, cell_points, cell_quotient, cell_quotient_schoolbook

SHAPES = [(1, 0), (1, 1), (3, 1), (4, 2), (6, 0), (5, 5), (6, 3)]


@pytest.mark.parametrize('log2_n', [1, 2, 3, 6])
def test_transform_against_horner(log2_n):
    rnd = random.Random(3000 + log2_n)
    n = 1 << log2_n
    coef = [rnd.randrange(R) for _ in range(n)]
    assert to_evals(coef, log2_n) == evals_of(coef, log2_n)
    assert to_coeffs(evals_of(coef, log2_n), log2_n) == coef
    for s in (coset_shift(log2_n), R - 1, rnd.randrange(1, R)):
        vals = to_evals(coef, log2_n, s)
        assert vals == [horner(coef, s * w % R) for w in roots(log2_n)]
        assert to_coeffs(vals, log2_n, s) == coef


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_cells_are_the_values_on_the_cells_points(log2_n, log2_cell):
    rnd = random.Random(3100 + 16 * log2_n + log2_cell)
    n, c = 1 << log2_n, 1 << log2_cell
    f = [rnd.randrange(R) for _ in range(n)]
    coef = to_coeffs(f, log2_n)
    got = cells(f, log2_n, log2_cell)
    assert len(got) == 2 * n // c and [v for cell in got[:n // c] for v in cell] == f          # the first half is the blob itself
    w2 = roots(log2_n + 1)          # the 2 N roots in bit-reversed order: the domain of the extension
    for k, cell in enumerate(got):
        pts = cell_points(k, log2_n, log2_cell)
        assert pts == w2[c * k:c * k + c]
        assert cell == [horner(coef, x) for x in pts]
        s = pow(cell_shift(k, log2_n, log2_cell), c, R)
        assert all(pow(x, c, R) == s for x in pts)          # X^c - s_k vanishes on the cell
    z = rnd.randrange(R)
    assert horner(coef, z) == eval_roots(f, z, log2_n)


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_recurrence_against_long_division(log2_n, log2_cell):
    rnd = random.Random(3200 + 16 * log2_n + log2_cell)
    n, c = 1 << log2_n, 1 << log2_cell
    coef = [rnd.randrange(R) for _ in range(n)]
    for k in sorted({0, 1, 2 * n // c - 1, rnd.randrange(2 * n // c)}):
        q = cell_quotient(coef, k, log2_n, log2_cell)
        q2, rem = cell_quotient_schoolbook(coef, k, log2_n, log2_cell)
        assert q == q2 and not any(q[n - c:])
        for x in cell_points(k, log2_n, log2_cell):          # the remainder is the cell's interpolant
            assert horner(rem, x) == horner(coef, x)
        z = rnd.randrange(R)
        assert (horner(q, z) * (pow(z, c, R) - pow(cell_shift(k, log2_n, log2_cell), c, R)) + horner(rem, z)) % R == horner(coef, z)


def test_omega_orders():
    for k in range(0, 14):
        w = omega(k)
        assert pow(w, 1 << k, R) == 1 and (k == 0 or pow(w, 1 << (k - 1), R) == R - 1)
