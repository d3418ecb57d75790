"""The recovery of blobs from half of their cells without a GPU: fr_recover_* of fr_exec.h -- the code kzg_recover_z_kernel and kzg_recover_kernel compile for the device -- on
the simulator (nbls_sim_kzg_recover: the host's slot maps, one lane per Z value, 512 lanes per blob, phase after phase) against the specification's route in Python integers
(kzg_recover_cases.py).  Bit-exact.  Shapes: log2_n 1 .. 12 with the log2_cell values 0, 3, 6 and log2_n that the bounds allow.  Where a blob has more than 256 cells (the
reference builds Z in O(M^2) and the lanes walk M / 2 factors for each of 3 M / 2 values) or more than 512 elements (Python's transforms of size 2 N) the patterns are walked
with the random blob and the structured blobs with one pattern; below that every pattern meets every blob."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, NON_CANONICAL
from kzg_cells_cases import to_evals, cells, rows
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, n_cells, recover, patterns, blobs_for

SHAPES = [(L, lc) for L in range(1, 13) for lc in sorted({0, 3, 6, L}) if lc <= L and L + 1 - lc <= 12]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_kzg_recover.argtypes = [u, u, sz, vp, vp, vp, vp, vp, vp]
    return lib


def ints(raw, k):
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'big') for i in range(k)]


def run(sim, log2_n, log2_cell, blobs, coefs=True, status=True):
    """blobs: (index list, list of cells) each -> (per blob the 2 N / c cells, per blob the N coefficients, statuses)"""
    n, N, c = len(blobs), 1 << log2_n, 1 << log2_cell
    off = [0]
    for idx, _ in blobs:
        off.append(off[-1] + len(idx))
    flat = [k for idx, _ in blobs for k in idx]
    raw = b''.join(rows(cell) for _, given in blobs for cell in given)
    out, co, st = C.create_string_buffer(64 * N * n), C.create_string_buffer(32 * N * n), C.create_string_buffer(n)
    rc = sim.nbls_sim_kzg_recover(log2_n, log2_cell, n, (C.c_uint32 * (n + 1))(*off), (C.c_uint32 * max(len(flat), 1))(*flat), raw, out, co if coefs else None,
                                  st if status else None)
    assert rc == 0
    v, w = ints(out.raw, 2 * N * n), ints(co.raw, N * n)
    got = [[v[2 * N * i + c * k:2 * N * i + c * k + c] for k in range(2 * N // c)] for i in range(n)]
    return got, [w[N * i:N * i + N] for i in range(n)], list(st.raw)


@pytest.mark.parametrize('log2_n,log2_cell', SHAPES)
def test_against_the_reference(sim, log2_n, log2_cell):
    rnd = random.Random(7000 + 16 * log2_n + log2_cell)
    m = n_cells(log2_n, log2_cell)
    blobs, pats = blobs_for(log2_n, log2_cell, rnd), patterns(log2_n, log2_cell, rnd)
    pairs = [(b, p) for b in blobs for p in pats] if m <= 256 and log2_n <= 9 else [(blobs[0], p) for p in pats[4:7] + pats[8:]] + [(b, pats[4]) for b in blobs[1:4]]
    if m >= 4096:          # (11,0): 6144 values of 2048 factors a blob
        pairs = [(blobs[0], pats[5])]
    want = {bname: cells(to_evals(coef, log2_n), log2_n, log2_cell) for bname, coef in {b[0]: b[1] for b, _ in pairs}.items()}
    calls = [(idx, [want[bname][k] for k in idx]) for (bname, _), (_, idx) in pairs]
    got, gc, st = run(sim, log2_n, log2_cell, calls)
    assert st == [0] * len(pairs)
    slow = log2_n > 7
    for i, ((bname, coef), (pname, idx)) in enumerate(pairs):
        assert got[i] == want[bname] and gc[i] == coef, (bname, pname)
        if not slow or i == 0:          # the reference itself, by the specification's route (test_kzg_recover_cases.py has it reproduce the blob for every pattern)
            assert recover(idx, calls[i][1], log2_n, log2_cell) == (0, got[i], gc[i]), (bname, pname)
    assert run(sim, log2_n, log2_cell, calls[:2], coefs=False, status=False)[0] == got[:2]


@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (2, 1), (5, 5), (6, 0), (8, 3), (9, 6), (10, 4)])
def test_refused_blobs_between_good_ones(sim, log2_n, log2_cell):
    rnd = random.Random(7100 + 16 * log2_n + log2_cell)
    m, n = n_cells(log2_n, log2_cell), 1 << log2_n
    coef = [rnd.randrange(R) for _ in range(n)]
    want = cells(to_evals(coef, log2_n), log2_n, log2_cell)
    half = rnd.sample(range(m), m // 2)
    more = half + [next(k for k in range(m) if k not in half)]
    take = lambda idx: [list(want[k % m]) for k in idx]
    good = (half, take(half))

    def changed(idx, e, j, v):
        g = take(idx)
        g[e][j] = v if v is not None else (g[e][j] + 1) % R
        return idx, g
    c = 1 << log2_cell
    cases = [('short', (half[:-1], take(half[:-1])), BAD_CELLS), ('twice', (half[1:] + [half[-1]] * 2, take(half[1:] + [half[-1]] * 2)), BAD_CELLS),
             ('index = M', (half[:-1] + [m], take(half[:-1] + [m])), BAD_CELLS), ('none', ([], []), BAD_CELLS),
             ('element = r', changed(half, len(half) - 1, c - 1, R), NON_CANONICAL), ('element = 2^256 - 1', changed(more, len(more) - 1, 0, M256), NON_CANONICAL),
             ('short and non-canonical', (half[:-1], [[R] * c for _ in half[:-1]]), BAD_CELLS), ('changed, half + 1', changed(more, 0, 0, None), INCONSISTENT),
             ('changed in the second half of the list', changed(more, len(more) - 1, c - 1, None), INCONSISTENT)]
    idx, g = changed(more, 0, 0, None)
    g[1][0] = R
    cases.append(('non-canonical and inconsistent', (idx, g), NON_CANONICAL))
    flip = changed(half, 0, 0, None)
    for name, bad, code in cases:
        got, gc, st = run(sim, log2_n, log2_cell, [good, bad, flip])
        assert st == [0, code, 0], name
        assert got[0] == want and gc[0] == coef, name
        assert got[1] == [[0] * c] * m and gc[1] == [0] * n, name
    # one changed element with exactly half of the cells: a polynomial all the same, the reference's
    assert (0, got[2], gc[2]) == recover(flip[0], flip[1], log2_n, log2_cell) and gc[2] != coef


def test_argument_rules(sim):
    x, out = bytes(64), C.create_string_buffer(256)
    off, idx = (C.c_uint32 * 2)(0, 2), (C.c_uint32 * 2)(0, 1)
    f = sim.nbls_sim_kzg_recover
    assert f(1, 0, 1, off, idx, x, out, None, None) == 0
    assert f(0, 0, 1, off, idx, x, out, None, None) == -1
    assert f(13, 6, 1, off, idx, x, out, None, None) == -1
    assert f(1, 2, 1, off, idx, x, out, None, None) == -1
    assert f(12, 0, 1, off, idx, x, out, None, None) == -1          # 2^13 cells: more than the table of roots holds
    assert f(1, 0, 1, None, idx, x, out, None, None) == -1
    assert f(1, 0, 1, off, None, x, out, None, None) == -1
    assert f(1, 0, 1, off, idx, None, out, None, None) == -1
    assert f(1, 0, 1, off, idx, x, None, None, None) == -1
    assert f(1, 0, 1, (C.c_uint32 * 2)(1, 2), idx, x, out, None, None) == -1
    assert f(1, 0, 2, (C.c_uint32 * 3)(0, 2, 1), idx, x, out, None, None) == -1
    assert f(1, 0, 0, None, None, None, None, None, None) == 0
    st = C.create_string_buffer(1)
    assert f(1, 0, 1, (C.c_uint32 * 2)(0, 0), None, None, out, None, st) == 0 and st.raw[0] == BAD_CELLS
