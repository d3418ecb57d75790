"""The transform over Fr, the cells and the quotient rows of the cell proofs without a GPU: fr_ntt_* / fr_cell_chain of fr_exec.h -- the code kzg_ntt_kernel and
kzg_cell_rows_kernel compile for the device -- on the simulator (nbls_sim_fr_ntt, nbls_sim_kzg_cells, nbls_sim_kzg_cell_rows: 512 lanes per polynomial, the same elements and
butterflies per lane, phase after phase) against Python integers (kzg_cells_cases.py).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, NON_CANONICAL, horner, eval_roots
from kzg_cells_cases import LANES, to_evals, to_coeffs, coset_shift, cells, cell_quotient, structured, rows

TO_COEFFS, TO_EVALS = 0, 1
ZERO_SHIFT = 5


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_fr_ntt.argtypes = [u, C.c_int, sz, vp, vp, vp, vp]
    lib.nbls_sim_kzg_cells.argtypes = [u, sz, vp, vp, vp, vp]
    lib.nbls_sim_kzg_cell_rows.argtypes = [u, u, sz, vp, vp]
    return lib


def ints(raw, k):
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'big') for i in range(k)]


def ntt(sim, log2_n, direction, polys, shifts=None, status=True):
    n, N = len(polys), 1 << log2_n
    out, st = C.create_string_buffer(max(32 * n * N, 1)), C.create_string_buffer(max(n, 1))
    rc = sim.nbls_sim_fr_ntt(log2_n, direction, n, b''.join(rows(f) for f in polys), None if shifts is None else rows(shifts), out, st if status else None)
    assert rc == 0
    v = ints(out.raw, n * N)
    return [v[i * N:(i + 1) * N] for i in range(n)], list(st.raw[:n])


def shifts_for(log2_n, rnd):
    return [('none', None), ('1', 1), ('g', coset_shift(log2_n)), ('r-1', R - 1), ('random', rnd.randrange(1, R))]


@pytest.mark.parametrize('log2_n', range(1, 13))
def test_both_directions_against_python(sim, log2_n):
    rnd = random.Random(4000 + log2_n)
    cases = structured(log2_n, rnd)
    polys = [f for _, f in cases]
    for sname, s in shifts_for(log2_n, rnd):
        sh = None if s is None else [s] * len(polys)
        want_e = [to_evals(f, log2_n, s or 1) for f in polys]
        want_c = [to_coeffs(f, log2_n, s or 1) for f in polys]
        got_e, st_e = ntt(sim, log2_n, TO_EVALS, polys, sh)
        got_c, st_c = ntt(sim, log2_n, TO_COEFFS, polys, sh)
        assert st_e == [0] * len(polys) and st_c == st_e, sname
        for (name, _), ge, we, gc, wc in zip(cases, got_e, want_e, got_c, want_c):
            assert ge == we, (name, sname, 'to values')
            assert gc == wc, (name, sname, 'to coefficients')


@pytest.mark.parametrize('log2_n', [1, 4, 9, 10, 12])
def test_one_polynomial_and_three_with_their_own_shifts(sim, log2_n):
    rnd = random.Random(4100 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    ss = [rnd.randrange(1, R), 1, coset_shift(log2_n)]
    for d, ref in ((TO_EVALS, to_evals), (TO_COEFFS, to_coeffs)):
        assert ntt(sim, log2_n, d, fs[:1]) == ([ref(fs[0], log2_n)], [0])
        got, st = ntt(sim, log2_n, d, fs, ss)
        assert st == [0, 0, 0] and got == [ref(f, log2_n, s) for f, s in zip(fs, ss)]
        assert ntt(sim, log2_n, d, fs, ss, status=False)[0] == got          # status == NULL


@pytest.mark.parametrize('log2_n', [2, 9, 11])
def test_round_trip_and_horner_at_a_random_point(sim, log2_n):
    rnd = random.Random(4200 + log2_n)
    n = 1 << log2_n
    f = [rnd.randrange(R) for _ in range(n)]
    for s in (None, rnd.randrange(1, R)):
        sh = None if s is None else [s]
        (coef,), _ = ntt(sim, log2_n, TO_COEFFS, [f], sh)
        (back,), _ = ntt(sim, log2_n, TO_EVALS, [coef], sh)
        assert back == f
    (coef,), _ = ntt(sim, log2_n, TO_COEFFS, [f])
    z = rnd.randrange(R)
    assert horner(coef, z) == eval_roots(f, z, log2_n)


@pytest.mark.parametrize('log2_n', [2, 9, 10])
@pytest.mark.parametrize('bad', ['element=r', 'element=2^256-1', 'shift=r', 'shift=0'])
def test_refused_inputs(sim, log2_n, bad):
    rnd = random.Random(4300 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    ss = [rnd.randrange(1, R) for _ in range(3)]
    for d, ref in ((TO_EVALS, to_evals), (TO_COEFFS, to_coeffs)):
        want = [ref(f, log2_n, s) for f, s in zip(fs, ss)]
        polys, sh, code = [list(f) for f in fs], list(ss), NON_CANONICAL
        if bad == 'shift=r':
            sh[1] = R
        elif bad == 'shift=0':
            sh[1], code = 0, ZERO_SHIFT
        else:
            polys[1][n - 1 if log2_n != 10 else LANES + 3] = R if bad == 'element=r' else M256
        got, st = ntt(sim, log2_n, d, polys, sh)
        assert st == [0, code, 0]
        assert got == [want[0], [0] * n, want[2]]          # the row is zero, the neighbours intact
        assert ntt(sim, log2_n, d, polys, sh, status=False)[0] == got


@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (2, 1), (6, 0), (5, 5), (8, 3), (10, 6), (12, 6)])
def test_cells_against_python(sim, log2_n, log2_cell):
    rnd = random.Random(4400 + 16 * log2_n + log2_cell)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]]
    fs[1][n // 2] = R          # a refused blob between two good ones
    out, coef, st = C.create_string_buffer(64 * n * 3), C.create_string_buffer(32 * n * 3), C.create_string_buffer(3)
    assert sim.nbls_sim_kzg_cells(log2_n, 3, b''.join(rows(f) for f in fs), out, coef, st) == 0
    assert list(st.raw) == [0, NON_CANONICAL, 0]
    for i, f in enumerate(fs):
        got, gc = ints(out.raw[64 * n * i:64 * n * (i + 1)], 2 * n), ints(coef.raw[32 * n * i:32 * n * (i + 1)], n)
        if i == 1:
            assert got == [0] * (2 * n) and gc == [0] * n
            continue
        assert got[:n] == f
        assert got == [v for cell in cells(f, log2_n, log2_cell) for v in cell]
        assert gc == to_coeffs(f, log2_n)


@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (1, 1), (3, 1), (4, 2), (6, 0), (5, 5), (8, 3)])
def test_cell_rows_against_python(sim, log2_n, log2_cell):
    rnd = random.Random(4500 + 16 * log2_n + log2_cell)
    n, m = 1 << log2_n, 2 << (log2_n - log2_cell)
    coefs = [[rnd.randrange(R) for _ in range(n)], [0] * n, [rnd.randrange(R) for _ in range(n)]]
    out = C.create_string_buffer(32 * n * m * 3)
    assert sim.nbls_sim_kzg_cell_rows(log2_n, log2_cell, 3, b''.join(rows(c) for c in coefs), out) == 0
    got = ints(out.raw, 3 * m * n)
    for i, coef in enumerate(coefs):
        for k in range(m):
            assert got[(i * m + k) * n:(i * m + k + 1) * n] == cell_quotient(coef, k, log2_n, log2_cell), (i, k)


def test_argument_rules(sim):
    x, out = bytes(64), C.create_string_buffer(256)
    assert sim.nbls_sim_fr_ntt(0, 0, 1, x, None, out, None) == -1
    assert sim.nbls_sim_fr_ntt(13, 0, 1, x, None, out, None) == -1
    assert sim.nbls_sim_fr_ntt(1, 2, 1, x, None, out, None) == -1
    assert sim.nbls_sim_fr_ntt(1, 0, 1, None, None, out, None) == -1
    assert sim.nbls_sim_fr_ntt(1, 0, 1, x, None, None, None) == -1
    assert sim.nbls_sim_fr_ntt(12, 1, 4097, None, None, None, None) == -1
    assert sim.nbls_sim_fr_ntt(1, 1, 0, None, None, None, None) == 0
    assert sim.nbls_sim_kzg_cell_rows(1, 2, 1, x, out) == -1
    assert sim.nbls_sim_kzg_cell_rows(12, 0, 1, x, out) == -1          # 2^13 rows: more than the table of roots holds
