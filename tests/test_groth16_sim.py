"""The weighted sums of Groth16 public inputs without a GPU: g16_* of fr_exec.h -- the code g16_input_sums_kernel compiles for the device -- on the simulator
(nbls_sim_g16_input_sums: the same tiles of 64 columns, row groups, unreduced accumulators, one reduction per lane, column tree and closing kernel) against Python integers
(groth16_cases.input_sums).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from groth16_cases import R, M256, NON_CANONICAL, ROWS_WG, GROUPS, MAX_WG, b32, input_sums

NS = [1, 2, ROWS_WG - 1, ROWS_WG, ROWS_WG + 1, 3 * ROWS_WG + 1]
MS = [1, 2, 63, 64, 65, 129]
W64 = (1 << 64) - 1


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz = C.c_void_p, C.c_size_t
    lib.nbls_sim_g16_input_sums.argtypes = [sz, sz, C.c_uint, vp, vp, vp, vp, vp]
    return lib


def run(sim, rows, weights, pre=None, n_wg=0, status=True, rc=0):
    n, m = len(rows), len(rows[0])
    out = C.create_string_buffer(32 * (m + 1))
    st = C.create_string_buffer(b'\x7f' * n, n)
    got = sim.nbls_sim_g16_input_sums(n, m, n_wg, b''.join(b32(x) for row in rows for x in row), b''.join(b32(w) for w in weights),
                                      None if pre is None else bytes(pre), out, st if status else None)
    assert got == rc
    return [int.from_bytes(out.raw[32 * j:32 * j + 32], 'big') for j in range(m + 1)], list(st.raw)


def mixed(n, m, rnd):
    """weights 1, 2^63, 2^64 - 1 and random; elements 0, 1, r - 1 and random"""
    ws = [rnd.choice([1, 1 << 63, W64, rnd.randrange(1 << 64)]) for _ in range(n)]
    rows = [[rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(m)] for _ in range(n)]
    return rows, ws


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('n', NS)
def test_sizes_against_python_integers(sim, n, m):
    rows, ws = mixed(n, m, random.Random(1000 * n + m))
    assert run(sim, rows, ws) == input_sums(rows, ws)


@pytest.mark.parametrize('value', [0, 1, R - 1])
@pytest.mark.parametrize('w', [1, 1 << 63, W64])
def test_constant_matrices(sim, value, w):
    n, m = ROWS_WG + 1, 65
    rows, ws = [[value] * m for _ in range(n)], [w] * n
    want = [n * w % R] + [n * w * value % R] * m
    assert run(sim, rows, ws) == (want, [0] * n)


def test_all_r_minus_1_at_the_largest_row_count_of_a_lane(sim):
    """every product is (2^64 - 1)(r - 1), the largest a canonical row has, and ONE workgroup takes all the rows: a lane adds 1024 of them before its one reduction -- what a
    lane meets in the largest call (2^24 rows of one input on 1024 workgroups of sixteen row groups).  The accumulator's bound (fr_exec.h: 2^32 rows) is far above it"""
    per_lane = (1 << 24) // (MAX_WG * GROUPS)
    n, m = per_lane * GROUPS, 2
    rows, ws = [[R - 1] * m] * n, [W64] * n
    want = [n * W64 % R] + [n * W64 * (R - 1) % R] * m
    assert run(sim, rows, ws, n_wg=1) == (want, [0] * n)
    assert run(sim, rows[:ROWS_WG * 3 + 1], ws[:ROWS_WG * 3 + 1])[0] == input_sums(rows[:ROWS_WG * 3 + 1], ws[:ROWS_WG * 3 + 1])[0]


def test_the_split_into_workgroups_does_not_change_a_byte(sim):
    rows, ws = mixed(3 * ROWS_WG + 1, 65, random.Random(77))
    want = input_sums(rows, ws)
    for n_wg in (1, 2, 3, 4, 7):
        assert run(sim, rows, ws, n_wg=n_wg) == want, n_wg


@pytest.mark.parametrize('m', [1, 64, 65, 129])
@pytest.mark.parametrize('bad', [R, M256])
def test_non_canonical_elements_take_their_row_out(sim, m, bad):
    n = 3 * ROWS_WG + 1
    for k, (i, j) in enumerate((i, j) for i in (0, n // 2, n - 1) for j in sorted({0, m - 1})):
        rows, ws = mixed(n, m, random.Random(300 + 10 * m + k))
        rows[i][j] = bad
        got = run(sim, rows, ws)
        assert got == input_sums(rows, ws), (i, j)
        assert got[1] == [NON_CANONICAL if r == i else 0 for r in range(n)]
        clean = [row for r, row in enumerate(rows) if r != i], [w for r, w in enumerate(ws) if r != i]
        assert got[0] == input_sums(*clean)[0]          # the neighbours are not disturbed


def test_pre_statuses_take_rows_out_and_are_copied(sim):
    n, m = 2 * ROWS_WG + 3, 65
    rows, ws = mixed(n, m, random.Random(41))
    pre = [0] * n
    for i, p in ((0, 3), (5, 13), (ROWS_WG, 34), (n - 1, 1)):
        pre[i] = p
    rows[5][m - 1] = R          # what came in stays the row's status
    rows[7][0] = R
    got = run(sim, rows, ws, pre=pre)
    assert got == input_sums(rows, ws, pre)
    assert got[1][0] == 3 and got[1][5] == 13 and got[1][7] == NON_CANONICAL and got[1][ROWS_WG] == 34 and got[1][n - 1] == 1


def test_every_row_out_gives_zero_sums(sim):
    rows, ws = mixed(5, 3, random.Random(5))
    assert run(sim, rows, ws, pre=[4] * 5) == ([0] * 4, [4] * 5)


def test_status_and_pre_may_be_null(sim):
    rows, ws = mixed(ROWS_WG + 1, 3, random.Random(6))
    rows[2][1] = R
    sums, st = run(sim, rows, ws, status=False)
    assert sums == input_sums(rows, ws)[0] and st == [0x7f] * len(rows)          # nothing written


def test_refusals(sim):
    rows, ws = mixed(2, 2, random.Random(7))
    run(sim, rows, [1 << 64, 1], rc=-1)          # a weight >= 2^64
    run(sim, rows, [1, 1 << 255], rc=-1)
    out = C.create_string_buffer(96)
    f = sim.nbls_sim_g16_input_sums
    x = b32(1)
    assert f(0, 2, 0, x * 4, x * 2, None, out, None) == -1 and f(2, 0, 0, x * 4, x * 2, None, out, None) == -1
    assert f(1 << 13, (1 << 11) + 1, 0, x, x, None, out, None) == -1          # n * m > 2^24: refused before anything is read
    assert f(2, 2, 0, None, x * 2, None, out, None) == -1 and f(2, 2, 0, x * 4, None, None, out, None) == -1 and f(2, 2, 0, x * 4, x * 2, None, None, None) == -1
