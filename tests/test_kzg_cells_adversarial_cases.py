"""The case builders of test_gpu_kzg_cells_adversarial.py check themselves in Python integers and against the oracle's points (no engine involved): an honest blob's cells and
the free-form tuples satisfy the integer form of the pairing equation, the model of the combined check accepts honest calls under several seeds and rejects a changed one, its
third flag is kzg_verify_cells_cases.neg_sums being all-zero, and every row of the zero-flag matrix reaches the flags stated for it."""
import hashlib
import random
import pytest
from kzg_cases import R, ZERO48, Setup, weight
from kzg_verify_cells_cases import random_blob, neg_sums
from kzg_cells_adversarial_cases import MATRIX, FORGED_ROWS, S_ROWS, Forge, values, call_args, matrix_rows

SEED = bytes(range(32))
SEEDS = [SEED, hashlib.sha256(b'kzg cells adversarial').digest(), bytes(32)]


@pytest.fixture(scope='module')
def setup(oracle):
    return Setup(oracle)


@pytest.mark.parametrize('shape', [(1, 0), (2, 1), (7, 6), (8, 3)])          # (not c = N, where every quotient is zero)
def test_honest_cells_hold_and_the_model_accepts_them(setup, shape):
    rnd = random.Random(9000 + 16 * shape[0] + shape[1])
    fg = Forge(setup, *shape)
    blobs = [random_blob(setup, *shape, rnd) for _ in range(2)]
    items = [fg.honest(blobs[j % 2], k) for j, k in enumerate([0, fg.m - 1, 1, fg.m // 2, 0])]
    assert all(fg.holds(t) for t in items) and len({t.C for t in items}) == 2
    for seed in SEEDS:
        flags, za, zb, ok = fg.model(items, seed)
        assert (flags, za, zb, ok) == ([False] * 3, False, False, True)
        w = [weight(seed, j) for j in range(len(items))]
        assert neg_sums([values(t.cell_bytes) for t in items], [t.k for t in items], w, *shape) != [0] * fg.c
    bad = list(items)
    bad[2] = fg.with_element(bad[2], fg.c - 1, 1)
    assert [fg.holds(t) for t in bad] == [True, True, False, True, True]
    assert all(not fg.model(bad, seed)[3] for seed in SEEDS)
    cs, ci, ki, cells, proofs = call_args(items)
    assert cs == [blobs[0].commitment, blobs[1].commitment] and ci == [0, 1, 0, 1, 0] and ki == [t.k for t in items]
    assert cells == [blobs[j % 2].cell(t.k) for j, t in enumerate(items)] and proofs == [blobs[j % 2].proof(t.k) for j, t in enumerate(items)]


@pytest.mark.parametrize('shape', [(1, 0), (8, 3), (7, 6)])
def test_free_form_tuples_hold(setup, shape):
    rnd = random.Random(9100 + shape[0])
    fg = Forge(setup, *shape)
    for k, q in ((0, rnd.randrange(1, R)), (fg.m - 1, rnd.randrange(1, R)), (1, 0)):
        v = [rnd.randrange(R) for _ in range(fg.c)]
        t = fg.tuple_for(k, v, q)
        assert fg.holds(t) and values(t.cell_bytes) == v and (t.P == ZERO48) == (q == 0)
        assert t.cm == (q * (fg.tau_c - fg.s(k)) + t.I) % R
        assert not fg.holds(fg.with_q(t, t.q + 1)) and not fg.holds(fg.with_cm(t, t.cm + 1)) and not fg.holds(fg.with_element(t, 0, 1))
        j, d = rnd.randrange(fg.c), rnd.randrange(1, R)
        assert fg.with_element(t, j, d).I == (t.I + d * fg.unit_at_tau(k, j)) % R          # what an added d is worth at tau
    a = [rnd.randrange(R) for _ in range(fg.c)]
    assert fg.coeffs(fg.tuple_for(2, fg.cell_with_coeffs(2, a), 5)) == a


@pytest.mark.parametrize('shape', [(1, 0), (8, 3)])
def test_matrix_rows_reach_their_flags(setup, shape):
    fg = Forge(setup, *shape)
    rows = matrix_rows(fg, SEED, random.Random(9200 + shape[0]))
    assert set(S_ROWS) < set(MATRIX) and FORGED_ROWS < set(MATRIX)
    for name, (flags, za, zb) in MATRIX.items():
        items = rows[name]
        got = fg.model(items, SEED)
        assert got[:3] == (flags, za, zb), name
        assert got[3] == (name not in FORGED_ROWS), name
        assert all(fg.holds(t) for t in items) == (name not in FORGED_ROWS), name
        assert all(ZERO48 not in (t.C, t.P) for t in items), name
        w = [weight(SEED, j) for j in range(len(items))]
        assert (neg_sums([values(t.cell_bytes) for t in items], [t.k for t in items], w, *shape) == [0] * fg.c) == flags[2], name
        # the rows are made for SEED's weights: under another seed only what all-zero cells give remains
        assert fg.model(items, SEEDS[1])[:3] == ([False, False, not any(any(values(t.cell_bytes)) for t in items)], False, False), name
