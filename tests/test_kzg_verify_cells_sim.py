"""The interpolation of cells without a GPU: fr_cell_* of fr_exec.h -- the code kzg_cell_interp_kernel compiles for the device -- on the simulator (nbls_sim_kzg_cell_interp:
workgroups of 256 lanes, c lanes per cell, a stage's partner read from the lane i ^ len, the kernel's column trees) against Python integers (kzg_verify_cells_cases.py).
Bit-exact, in the rows mode and in the sum mode."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, NON_CANONICAL, b32
from kzg_verify_cells_cases import LANES, WALK, cells_per_blob, neg_rows, neg_sums, cell_bytes

PAIRS = [(n, c) for c in range(7) for n in sorted({c, 7, 12}) if n >= 1 and n + 1 - c <= 12]          # (0, 0) and (12, 0) are refused: no blob of one element, 2^13 cells per blob
WEIGHTS = [1 << 63, (1 << 64) - 1, 0]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_kzg_cell_interp.argtypes = [u, u, sz, C.c_int, u, vp, vp, vp, vp, vp, vp]
    return lib


def run(sim, log2_n, log2_cell, cell_list, idx, weights=None, pre=None, n_wg=0, status=True):
    """-> (rows of c integers: one per cell in the rows mode (weights None), else the one row of the -S_i; statuses)"""
    n, c = len(cell_list), 1 << log2_cell
    out = C.create_string_buffer(32 * c * (n if weights is None else 1))
    st = C.create_string_buffer(b'\x7f' * n, n)
    rc = sim.nbls_sim_kzg_cell_interp(log2_n, log2_cell, n, 0 if weights is None else 1, n_wg, b''.join(cell_bytes(v) for v in cell_list), (C.c_uint32 * n)(*idx),
                                      None if pre is None else bytes(pre), None if weights is None else b''.join(b32(w) for w in weights), out, st if status else None)
    assert rc == 0
    v = [int.from_bytes(out.raw[32 * i:32 * i + 32], 'big') for i in range(len(out.raw) // 32)]
    return [v[i * c:(i + 1) * c] for i in range(len(v) // c)], list(st.raw)


def structured(c, rnd):
    one = lambda j: [rnd.randrange(1, R) if i == j else 0 for i in range(c)]
    return [[0] * c, [rnd.randrange(1, R)] * c, [R - 1] * c, one(0), one(c - 1), [rnd.randrange(R) for _ in range(c)]]


@pytest.mark.parametrize('log2_n,log2_cell', PAIRS)
def test_structured_cells_both_modes(sim, log2_n, log2_cell):
    rnd = random.Random(7300 + 16 * log2_n + log2_cell)
    c, m = 1 << log2_cell, cells_per_blob(log2_n, log2_cell)
    cell_list = structured(c, rnd)
    places = [0, 1, m - 1, m // 2]
    idx = [places[j % 4] for j in range(len(cell_list))]
    for k in places:          # and a random cell at every one of the four places
        cell_list.append([rnd.randrange(R) for _ in range(c)])
        idx.append(k)
    w = [WEIGHTS[j % 3] for j in range(len(cell_list))]
    w[-1] = rnd.getrandbits(64) | 1 << 63
    rows, st = run(sim, log2_n, log2_cell, cell_list, idx)
    assert st == [0] * len(cell_list)
    assert rows == neg_rows(cell_list, idx, log2_n, log2_cell)
    want = neg_sums(cell_list, idx, w, log2_n, log2_cell)
    for n_wg in (0, 1, 3):          # the launcher's count; one workgroup (c = 64: four lane groups walk the ten cells); three partial rows
        got, st = run(sim, log2_n, log2_cell, cell_list, idx, weights=w, n_wg=n_wg)
        assert got == [want] and st == [0] * len(cell_list), n_wg
    assert run(sim, log2_n, log2_cell, cell_list, idx, weights=w, status=False)[0] == [want]          # st_out == NULL


@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (7, 0), (2, 1), (7, 3), (12, 5), (7, 6), (12, 6)])
def test_counts_that_leave_groups_empty_and_walk_several_cells(sim, log2_n, log2_cell):
    """2 * (cells a workgroup holds) + 3 cells: with one workgroup every lane group walks three rounds, the last of them on three cells only; with the launcher's count the last
    workgroup is partly empty; one cell alone leaves every other group of its wavefront empty"""
    rnd = random.Random(7400 + 16 * log2_n + log2_cell)
    c, m, per_wg = 1 << log2_cell, cells_per_blob(log2_n, log2_cell), LANES >> log2_cell
    pool = [[rnd.randrange(R) for _ in range(c)] for _ in range(5)]
    for n in (1, 2 * per_wg + 3, WALK * per_wg + 1):
        pick = [rnd.randrange(5) for _ in range(n)]
        cell_list, idx = [pool[j] for j in pick], [(7 * j + pick[j]) % m for j in range(n)]
        w = [rnd.getrandbits(64) | 1 << 63 for _ in range(n)]
        assert run(sim, log2_n, log2_cell, cell_list, idx)[0] == neg_rows(cell_list, idx, log2_n, log2_cell), n
        want = neg_sums(cell_list, idx, w, log2_n, log2_cell)
        for n_wg in (0, 1, 2):
            assert run(sim, log2_n, log2_cell, cell_list, idx, weights=w, n_wg=n_wg)[0] == [want], (n, n_wg)


@pytest.mark.parametrize('log2_n,log2_cell', PAIRS)
def test_refused_cells_between_good_ones(sim, log2_n, log2_cell):
    rnd = random.Random(7500 + 16 * log2_n + log2_cell)
    c, m = 1 << log2_cell, cells_per_blob(log2_n, log2_cell)
    cell_list = [[rnd.randrange(R) for _ in range(c)] for _ in range(7)]
    idx = [rnd.randrange(m) for _ in range(7)]
    cell_list[1][c - 1] = R
    cell_list[3][c // 2] = M256
    pre = [0, 0, 0, 0, 0, 13, 0]          # a cell the decoders refused: out, and its status passes through
    w = [rnd.getrandbits(64) | 1 << 63 for _ in range(7)]
    out = {1, 3, 5}
    want_st = [0, NON_CANONICAL, 0, NON_CANONICAL, 0, 13, 0]
    rows, st = run(sim, log2_n, log2_cell, cell_list, idx, pre=pre)
    good = [[v % R for v in cell] for cell in cell_list]          # (the refused cells' rows are zero whatever they hold)
    assert st == want_st and rows == neg_rows(good, idx, log2_n, log2_cell, out=out)
    for n_wg in (0, 1):
        got, st = run(sim, log2_n, log2_cell, cell_list, idx, weights=w, pre=pre, n_wg=n_wg)
        assert st == want_st and got == [neg_sums(good, idx, w, log2_n, log2_cell, out=out)]
    pre[1] = 4          # a decoder's status goes in front of the canonical check's
    assert run(sim, log2_n, log2_cell, cell_list, idx, pre=pre)[1] == [0, 4, 0, NON_CANONICAL, 0, 13, 0]


def test_argument_rules(sim):
    x, one, out = bytes(64 * 32), (C.c_uint32 * 1)(0), C.create_string_buffer(64 * 32)
    f = sim.nbls_sim_kzg_cell_interp
    assert f(0, 0, 1, 0, 0, x, one, None, None, out, None) == -1          # no blob of one element
    assert f(12, 0, 1, 0, 0, x, one, None, None, out, None) == -1         # 2^13 cells per blob
    assert f(7, 7, 1, 0, 0, x, one, None, None, out, None) == -1          # log2_cell > 6
    assert f(3, 4, 1, 0, 0, x, one, None, None, out, None) == -1          # log2_cell > log2_n
    assert f(3, 1, 0, 0, 0, x, one, None, None, out, None) == -1          # no cell
    assert f(3, 1, 1, 1, 0, x, one, None, None, out, None) == -1          # the sum mode without weights
    assert f(3, 1, 1, 0, 0, x, (C.c_uint32 * 1)(8), None, None, out, None) == -1          # cell_index = 2 N / c
    assert f(3, 1, 1, 0, 0, x, (C.c_uint32 * 1)(7), None, None, out, None) == 0
