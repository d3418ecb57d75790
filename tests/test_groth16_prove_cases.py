"""The construction of the Groth16 prover's tests checked before anything is compared with it (no GPU): the instances groth16_prove_cases.py makes are satisfied, the
quotient in Python integers satisfies h(tau) Z(tau) = (Az)(tau) (Bz)(tau) - (Cz)(tau) with a zero top coefficient, and the proof scalars of the trapdoor key satisfy the
verifier's equation a b = alpha beta + gamma l + delta c (Key.holds_scalars) for the public inputs z_1 .. z_m."""
import random
import pytest
from groth16_cases import ZERO96
from groth16_prove_cases import R, ZERO48, instance, family, matvec, bitrev_order, quotient, poly_at, ProvingKey


@pytest.fixture(scope='module', params=[(1, 4, 1), (2, 5, 2), (4, 20, 3), (6, 70, 4)], ids=str)
def case(request, oracle):
    log2_n, n_vars, m = request.param
    rnd = random.Random(1700 + log2_n)
    A, B, Cm, z = instance(log2_n, n_vars, m, rnd)
    return log2_n, m, (A, B, Cm), z, ProvingKey(oracle, log2_n, n_vars, m, (A, B, Cm), rnd), rnd


def test_instances_are_satisfied(case):
    log2_n, _, mats, z, _, _ = case
    a, b, c = (matvec(M, z, log2_n) for M in mats)
    assert z[0] == 1 and all(x * y % R == w for x, y, w in zip(a, b, c)) and any(a) and any(b)


def test_a_family_has_many_witnesses_and_zero_query_points(oracle):
    rnd = random.Random(1699)
    A, B, Cm, witness = family(3, 6, 7, rnd, skip=(4,))
    key = ProvingKey(oracle, 3, 13, 2, (A, B, Cm), rnd)
    zs = [witness(rnd) for _ in range(3)]
    assert zs[0] != zs[1]
    for z in zs:
        a, b, c = (matvec(M, z, 3) for M in (A, B, Cm))
        assert all(x * y % R == w for x, y, w in zip(a, b, c))
        assert key.holds_scalars(key.proof_scalars(z, rnd.randrange(R), rnd.randrange(R)), z[1:3])
    # the variables a row writes are named by C alone; column 4 by nothing
    assert all(key.at[0][i] == 0 and key.at[1][i] == 0 and key.at[2][i] for i in range(6, 13)) and key.k[4] == 0
    assert key.points()['a_query48'][6] == ZERO48 and key.points()['l_query48'][4 - 3] == ZERO48 and key.points()['b_g2_query96'][12] == ZERO96


def test_quotient_identity_and_top_coefficient(case):
    log2_n, _, mats, z, key, _ = case
    a, b, c = (bitrev_order(matvec(M, z, log2_n), log2_n) for M in mats)
    h = quotient(a, b, c, log2_n)
    assert len(h) == 1 << log2_n and h[-1] == 0
    az, bz, cz = (sum(x * y for x, y in zip(col, z)) % R for col in key.at)
    assert poly_at(h, key.tau) * key.zt % R == (az * bz - cz) % R


def test_column_polynomials_interpolate_the_products(case):
    log2_n, _, mats, z, key, _ = case
    # sum_i z_i A_i(tau) is the interpolant of A z at tau: sum_j (Az)_j L_j(tau)
    for M, col in zip(mats, key.at):
        assert sum(x * y for x, y in zip(col, z)) % R == sum(v * l for v, l in zip(matvec(M, z, log2_n), key.lagrange)) % R


def test_proof_scalars_satisfy_the_verifier(case):
    _, m, _, z, key, rnd = case
    for r, s in ((rnd.randrange(R), rnd.randrange(R)), (0, 0), (R - 1, 1)):
        abc = key.proof_scalars(z, r, s)
        assert key.holds_scalars(abc, z[1:m + 1])
        assert not key.holds_scalars(abc, [(z[1] + 1) % R] + z[2:m + 1])
    assert key.proof_scalars(z, key.r_for_zero_a(z), 5)[0] == 0
