"""The recovery reference of kzg_recover_cases.py against what it must reproduce: the cells of the original blob (kzg_cells_cases.cells) from every index pattern, and the
refused inputs by construction.  Python integers only; nothing here touches the code under test."""
import random
import pytest
from kzg_cases import R, M256, NON_CANONICAL
from kzg_cells_cases import to_evals, cells
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, n_cells, cell_root, indices_ok, vanishing, recover_coeffs, recover, patterns, blobs_for

SHAPES = [(1, 0), (1, 1), (2, 1), (3, 1), (4, 2), (6, 3), (5, 0), (4, 4), (5, 5), (7, 6)]


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_reference_reproduces_the_blob(log2_n, log2_cell):
    rnd = random.Random(6000 + 16 * log2_n + log2_cell)
    for bname, coef in blobs_for(log2_n, log2_cell, rnd):
        want = cells(to_evals(coef, log2_n), log2_n, log2_cell)
        for pname, idx in patterns(log2_n, log2_cell, rnd):
            assert indices_ok(idx, log2_n, log2_cell), pname
            given = [want[k] for k in idx]
            assert recover_coeffs(idx, given, log2_n, log2_cell) == coef, (bname, pname)
            assert recover(idx, given, log2_n, log2_cell) == (0, want, coef), (bname, pname)


def test_mainnet_once():
    rnd = random.Random(6100)
    coef = [rnd.randrange(R) for _ in range(4096)]
    want = cells(to_evals(coef, 12), 12, 6)
    idx = rnd.sample(range(128), 64)
    assert recover(idx, [want[k] for k in idx], 12, 6) == (0, want, coef)


@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (4, 2), (6, 0), (6, 3)])
def test_vanishing_polynomial_is_constant_on_every_cell(log2_n, log2_cell):
    rnd = random.Random(6200 + 16 * log2_n + log2_cell)
    m, c = n_cells(log2_n, log2_cell), 1 << log2_cell
    missing = rnd.sample(range(m), m // 2)
    zv = to_evals(vanishing(missing, log2_n, log2_cell), log2_n + 1)
    for k in range(m):
        zs = 1
        for j in missing:
            zs = zs * (cell_root(k, log2_n, log2_cell) - cell_root(j, log2_n, log2_cell)) % R
        assert zv[c * k:c * k + c] == [zs] * c
        assert (zs == 0) == (k in missing)


@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (5, 5), (6, 3), (6, 0)])
def test_refused_inputs(log2_n, log2_cell):
    rnd = random.Random(6300 + 16 * log2_n + log2_cell)
    m, n = n_cells(log2_n, log2_cell), 1 << log2_n
    coef = [rnd.randrange(R) for _ in range(n)]
    want = cells(to_evals(coef, log2_n), log2_n, log2_cell)
    half = sorted(rnd.sample(range(m), m // 2))
    take = lambda idx: [list(want[k % m]) for k in idx]
    # the index rules
    for idx in (half[:-1], half[1:] + [half[-1]] * 2, half[:-1] + [m], half + [half[0]], []):
        assert recover(idx, take(idx), log2_n, log2_cell)[0] == BAD_CELLS, idx
    # the canonical check, behind the index rules
    for bad in (R, M256):
        g = take(half)
        g[-1][-1] = bad
        assert recover(half, g, log2_n, log2_cell)[0] == NON_CANONICAL
        assert recover(half[:-1], [g[-1]] * (len(half) - 1), log2_n, log2_cell)[0] == BAD_CELLS
    # one changed element: exactly half still interpolates, half + 1 does not
    g = take(half)
    g[0][0] = (g[0][0] + 1) % R
    st, out, got = recover(half, g, log2_n, log2_cell)
    assert st == 0 and got != coef and [out[k] for k in half] == g
    more = half + [next(k for k in range(m) if k not in half)]
    g = take(more)
    g[0][0] = (g[0][0] + 1) % R
    assert recover(more, g, log2_n, log2_cell)[0] == INCONSISTENT
    g[1][0] = R          # non-canonical wins over inconsistent
    assert recover(more, g, log2_n, log2_cell)[0] == NON_CANONICAL
