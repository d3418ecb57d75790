"""The construction of the Groth16 tests checked before anything is compared with it (no GPU): the proofs groth16_cases.Key makes satisfy the single-proof equation under the
oracle's pairings, and the three spoilings the device tests rely on break it."""
import random
import pytest
from groth16_cases import R, Key


@pytest.fixture(scope='module')
def case(oracle):
    rnd = random.Random(1600)
    key = Key(oracle, 2, rnd)
    xs = [[rnd.randrange(R) for _ in range(2)] for _ in range(3)]
    return key, xs, [key.prove(x, rnd) for x in xs]


def test_valid_proofs_satisfy_the_equation(case):
    key, xs, proofs = case
    for abc, x in zip(proofs, xs):
        assert key.holds_scalars(abc, x) and key.holds_pairing_scalars(abc, x)


def test_wrong_input_is_rejected(case):
    key, xs, proofs = case
    for abc, x in zip(proofs, xs):
        spoiled = [(x[0] + 1) % R, x[1]]
        assert not key.holds_scalars(abc, spoiled) and not key.holds_pairing_scalars(abc, spoiled)


def test_swapped_a_is_rejected(case):
    key, xs, proofs = case
    (a0, b0, c0), (a1, b1, c1) = proofs[0], proofs[1]
    assert not key.holds_pairing_scalars((a1, b0, c0), xs[0]) and not key.holds_pairing_scalars((a0, b1, c1), xs[1])


def test_shifted_c_pair_is_rejected_singly_though_its_unweighted_product_holds(case):
    key, xs, proofs = case
    d = 0x1234567
    (a0, b0, c0), (a1, b1, c1) = proofs[0], proofs[1]
    p0, p1 = (a0, b0, (c0 + d) % R), (a1, b1, (c1 - d) % R)
    assert not key.holds_pairing_scalars(p0, xs[0]) and not key.holds_pairing_scalars(p1, xs[1])
    # e(C_0 + D, -delta) e(C_1 - D, -delta) = e(C_0, -delta) e(C_1, -delta): the product of the two equations still holds -- what the weights are there to catch
    total = sum(a * b - key.alpha * key.beta - key.gamma * key.l_scalar(x) - key.delta * c for (a, b, c), x in ((p0, xs[0]), (p1, xs[1])))
    assert total % R == 0


def test_zero_l_rows(case, oracle):
    key = case[0]
    rnd = random.Random(1601)
    x = key.inputs_for_zero_l(rnd)
    abc = key.prove(x, rnd)
    assert key.holds_pairing_scalars(abc, x) and not key.holds_pairing_scalars((abc[0], abc[1], (abc[2] + 1) % R), x)
