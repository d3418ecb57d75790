"""The identities the large transform rests on (fr_exec.h; nbls.h at nbls_fr_ntt_large), in Python integers against kzg_cells_cases.to_evals -- the textbook network that
test_kzg_cells_cases.py checks against Horner's rule.  Calls no code under test."""
import random
import pytest
from kzg_cases import R, bitrev
from kzg_cells_cases import omega, to_evals, to_coeffs
from fr_ntt_large_cases import table, stage, global_stages, run_stages, block_shift, split_runs, compose_to_evals, compose_to_coeffs, sparse_eval

SPLITS = [(6, 3), (7, 2), (5, 4)]


def poly(log2_n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(1 << log2_n)]


@pytest.mark.parametrize('log2_n', [3, 6])
def test_the_network_stage_by_stage_is_the_transform(log2_n):
    a, tab = poly(log2_n, 1), table(log2_n)
    want = to_evals(a, log2_n)
    for j in range(log2_n):
        stage(a, log2_n, j, tab)
    assert a == want


@pytest.mark.parametrize('log2_n,t', SPLITS)
def test_fact_1_the_table_of_2_to_the_k_roots_is_a_prefix(log2_n, t):
    k, big = log2_n - t, table(log2_n)
    assert big[:1 << k] == table(k)
    inv = [pow(x, -1, R) for x in big]
    assert inv[:1 << k] == [pow(x, -1, R) for x in table(k)]
    a = poly(log2_n, 2)
    by_big = list(a)
    for j in range(k):
        assert max(2 * blk for blk in range(1 << j)) < 1 << k
        stage(by_big, log2_n, j, big)
    assert global_stages(a, log2_n, k) == by_big


@pytest.mark.parametrize('log2_n,t', SPLITS)
def test_fact_2_the_first_k_stages_are_column_transforms(log2_n, t):
    k, a = log2_n - t, poly(log2_n, 3)
    got = global_stages(a, log2_n, k)
    for c in range(1 << t):
        assert got[c::1 << t] == to_evals(a[c::1 << t], k), c


@pytest.mark.parametrize('log2_n,t', SPLITS)
def test_fact_3_the_rest_is_the_shifted_transform_of_every_block(log2_n, t):
    k, a, tab = log2_n - t, poly(log2_n, 4), table(log2_n)
    want, mid = to_evals(a, log2_n), global_stages(a, log2_n, k)
    for b in range(1 << k):
        s = block_shift(log2_n, t, b)
        assert pow(s, 1 << t, R) == tab[b]
        # block b holds p mod (X^(2^t) - T_N[b])
        rem = [0] * (1 << t)
        zp = 1
        for i, c in enumerate(a):
            if i and i % (1 << t) == 0:
                zp = zp * tab[b] % R
            rem[i % (1 << t)] = (rem[i % (1 << t)] + c * zp) % R
        assert mid[b << t:(b + 1) << t] == rem, b
        assert to_evals(rem, t, s) == want[b << t:(b + 1) << t], b


@pytest.mark.parametrize('log2_n,t', SPLITS)
@pytest.mark.parametrize('shift', [1, 7, R - 1])
def test_the_composition_both_ways(log2_n, t, shift):
    a = poly(log2_n, 5)
    assert compose_to_evals(a, log2_n, t, shift) == to_evals(a, log2_n, shift)
    assert compose_to_coeffs(a, log2_n, t, shift) == to_coeffs(a, log2_n, shift)


@pytest.mark.parametrize('p', [1, 2, 3])
def test_runs_of_stages_are_independent_networks_over_the_row_bits(p):
    log2_n, t = 8, 2
    k, a = log2_n - t, poly(log2_n, 6)
    runs = split_runs(k, p)
    assert runs[0][0] == 0 and runs[-1][1] == k and all(x[1] == y[0] for x, y in zip(runs, runs[1:]))
    assert max(j1 - j0 for j0, j1 in runs) == p and min(j1 - j0 for j0, j1 in runs) >= p - 1 and len(runs) == -(-k // p)
    got, tab = list(a), table(k)
    for j0, j1 in runs:
        run_stages(got, log2_n, j0, j1, tab)
    assert got == global_stages(a, log2_n, k)


def test_split_runs_shapes():
    assert split_runs(12, 6) == [(0, 6), (6, 12)]
    assert split_runs(10, 6) == [(0, 5), (5, 10)]
    assert split_runs(3, 1) == [(0, 1), (1, 2), (2, 3)]
    assert split_runs(5, 9) == [(0, 5)]
    assert split_runs(11, 4) == [(0, 4), (4, 8), (8, 11)]


def test_sparse_closed_form():
    log2_n = 7
    terms = [(0, 3), (5, R - 2), (64, 11), (127, 1)]
    coef = [0] * (1 << log2_n)
    for e, c in terms:
        coef[e] = c
    for shift in (1, 7):
        want = to_evals(coef, log2_n, shift)
        assert [sparse_eval(terms, log2_n, j, shift) for j in range(1 << log2_n)] == want
    assert pow(omega(log2_n), bitrev(1, log2_n), R) == R - 1
