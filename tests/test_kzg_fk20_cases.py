"""The identities of FK20 (kzg_fk20_cases.py) in Python integers against the quotient recurrence of kzg_cells_cases.py with tau known: what the device calls and the
simulator are then held to.  No code under test runs here."""
import random

import pytest

from kzg_cases import R, horner
from kzg_cells_cases import cell_quotient
import kzg_fk20_cases as fk

SIZES = [(1, 0), (1, 1), (2, 1), (2, 2), (5, 0), (5, 2), (5, 5), (6, 3)]
TAU = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % R


def _poly(log2_n, log2_cell):
    rnd = random.Random(7594 * 64 + 8 * log2_n + log2_cell)
    return [rnd.randrange(R) for _ in range(1 << log2_n)]


def _expected(coef, log2_n, log2_cell):
    M = fk.dims(log2_n, log2_cell)[3]
    return [horner(cell_quotient(coef, k, log2_n, log2_cell), TAU) for k in range(M)]


@pytest.mark.parametrize('log2_n,log2_cell', SIZES)
def test_identity_1_proof_is_a_sum_over_h(log2_n, log2_cell):
    coef = _poly(log2_n, log2_cell)
    _, _, np_, M, _ = fk.dims(log2_n, log2_cell)
    h = [fk.h_direct(coef, u, TAU, log2_n, log2_cell) for u in range(np_ - 1)]
    got = [sum(pow(fk.s_of(k, log2_n, log2_cell), u, R) * h[u] for u in range(np_ - 1)) % R for k in range(M)]
    assert got == _expected(coef, log2_n, log2_cell)


@pytest.mark.parametrize('log2_n,log2_cell', SIZES)
def test_identities_2_and_3_h_from_the_pointwise_products(log2_n, log2_cell):
    coef = _poly(log2_n, log2_cell)
    _, _, np_, M, lm = fk.dims(log2_n, log2_cell)
    y = fk.idft(fk.yhat(coef, TAU, log2_n, log2_cell), lm)
    assert [y[np_ - 1 + u] for u in range(np_ - 1)] == [fk.h_direct(coef, u, TAU, log2_n, log2_cell) for u in range(np_ - 1)]


@pytest.mark.parametrize('log2_n,log2_cell', SIZES)
def test_identity_4_projection_matrix(log2_n, log2_cell):
    coef = _poly(log2_n, log2_cell)
    assert fk.proofs_fk20(coef, TAU, log2_n, log2_cell) == _expected(coef, log2_n, log2_cell)


def test_one_cell_per_half_has_only_zero_proofs():
    """c = N: every sum is empty, the matrix is zero"""
    assert fk.matrix(5, 5) == [[0, 0], [0, 0]] and fk.proofs_fk20(_poly(5, 5), TAU, 5, 5) == [0, 0]


def test_degree_below_c_has_nonzero_products_and_zero_proofs():
    """what pass B must send to the exact zero point: y^ is not zero, every proof is"""
    coef = _poly(5, 2)[:4] + [0] * 28
    assert any(fk.yhat(coef, TAU, 5, 2)) and fk.proofs_fk20(coef, TAU, 5, 2) == [0] * 16


def test_flat_order_is_position_major():
    coef = _poly(5, 2)
    a, flat = fk.scalars(coef, 5, 2), fk.scalars_flat(coef, 5, 2)
    assert flat[3 * 4 + 1] == a[1][3] and len(flat) == 64
