"""The workgroup bodies of fr_workgroup.h -- the choreography kzg_kernels.hip and groth16_kernels.hip compile for the device: phases between barriers, the tree, the shared
flags, the uniform exits -- on the simulator's workgroup view, with the lanes of every phase visited from lane 0 up and from the top down (nbls_sim_set_lane_order).  Within
a phase the lanes are independent by construction, so a result that depends on the order is a missing barrier in the single source.  Every entry point that runs a shared body
is called in both orders: the outputs are byte-identical and equal the Python-integer references of the entry point's own test file.  Shapes: the smallest at which a body
has all its cases (idle lanes, more than one element a lane, more than one workgroup, every uniform exit)."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, NON_CANONICAL, b32, roots, eval_roots
from kzg_prove_cases import quotient
from kzg_cells_cases import to_evals, to_coeffs, cells, rows
from kzg_fk20_cases import scalars_flat
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, n_cells
from kzg_verify_cells_cases import interp_coeffs, cell_bytes
from groth16_cases import input_sums


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_set_lane_order.argtypes = [C.c_int]
    lib.nbls_sim_set_lane_order.restype = None
    lib.nbls_sim_fr_eval_roots.argtypes = [u, sz, vp, vp, vp, vp]
    lib.nbls_sim_fr_quotient_roots.argtypes = [u, sz, vp, vp, vp, vp, vp]
    lib.nbls_sim_fr_ntt.argtypes = [u, C.c_int, sz, vp, vp, vp, vp]
    lib.nbls_sim_kzg_cells.argtypes = [u, sz, vp, vp, vp, vp]
    lib.nbls_sim_kzg_canon.argtypes = [u, sz, vp, vp]
    lib.nbls_sim_kzg_sum.argtypes = [sz, vp, vp]
    lib.nbls_sim_kzg_fk20_scalars.argtypes = [u, u, sz, vp, vp]
    lib.nbls_sim_kzg_recover.argtypes = [u, u, sz, vp, vp, vp, vp, vp, vp]
    lib.nbls_sim_kzg_cell_interp.argtypes = [u, u, sz, C.c_int, u, vp, vp, vp, vp, vp, vp]
    lib.nbls_sim_g16_input_sums.argtypes = [sz, sz, u, vp, vp, vp, vp, vp]
    yield lib
    lib.nbls_sim_set_lane_order(0)


def ints(raw):
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'big') for i in range(len(raw) // 32)]


def both_orders(sim, call):
    """call() -> the output bytes of one simulator call; run with the lanes ascending, then descending"""
    try:
        sim.nbls_sim_set_lane_order(0)
        up = call()
        sim.nbls_sim_set_lane_order(1)
        down = call()
    finally:
        sim.nbls_sim_set_lane_order(0)
    assert up == down, 'the result depends on the order of the lanes within a phase: a barrier is missing'
    return up


# log2_n = 1: 254 idle lanes under the mask; 9: two terms a lane.  z off the roots, on a root (the lane that owns it: the first, one in the second term of its lane), and
# a non-canonical element / point
@pytest.mark.parametrize('log2_n', [1, 9])
def test_evaluation_and_quotient(sim, log2_n):
    rnd = random.Random(9100 + log2_n)
    n = 1 << log2_n
    w = roots(log2_n)
    f = [rnd.randrange(R) for _ in range(n)]
    bad = list(f)
    bad[n - 1] = R
    polys = [f, f, f, bad, f]
    zs = [rnd.randrange(R), w[0], w[n - 1], rnd.randrange(R), M256]
    k = len(polys)
    fb, zb = b''.join(b32(v) for p in polys for v in p), b''.join(map(b32, zs))

    def evaluate():
        out, st = C.create_string_buffer(32 * k), C.create_string_buffer(k)
        assert sim.nbls_sim_fr_eval_roots(log2_n, k, fb, zb, out, st) == 0
        return out.raw + st.raw

    def divide():
        y, q, st = C.create_string_buffer(32 * k), C.create_string_buffer(32 * n * k), C.create_string_buffer(k)
        assert sim.nbls_sim_fr_quotient_roots(log2_n, k, fb, zb, y, q, st) == 0
        return y.raw + q.raw + st.raw
    want = [quotient(p, z, log2_n) for p, z in zip(polys[:3], zs[:3])]
    got = both_orders(sim, evaluate)
    assert ints(got[:32 * k]) == [y for y, _ in want] + [0, 0] and list(got[32 * k:]) == [0, 0, 0, NON_CANONICAL, NON_CANONICAL]
    assert [y for y, _ in want] == [eval_roots(p, z, log2_n) for p, z in zip(polys[:3], zs[:3])]
    got = both_orders(sim, divide)
    assert ints(got[:32 * k]) == [y for y, _ in want] + [0, 0] and list(got[-k:]) == [0, 0, 0, NON_CANONICAL, NON_CANONICAL]
    assert ints(got[32 * k:-k]) == [v for _, q in want for v in q] + [0] * (2 * n)


# log2_n = 1: 511 idle lanes; 10: two elements a lane.  Both directions with and without shifts, a shift that is zero and one that is >= r (refused: the early exit), a
# non-canonical element, and the cells mode with the coefficients kept
@pytest.mark.parametrize('log2_n', [1, 10])
def test_transform_all_modes(sim, log2_n):
    rnd = random.Random(9200 + log2_n)
    n = 1 << log2_n
    f = [rnd.randrange(R) for _ in range(n)]
    bad = list(f)
    bad[n // 2] = M256
    s = rnd.randrange(1, R)
    polys, shifts = [f, f, f, bad], [s, 0, R, s]
    pb, sb = b''.join(rows(p) for p in polys), rows(shifts)

    def ntt(direction, shift):
        def call():
            out, st = C.create_string_buffer(32 * n * 4), C.create_string_buffer(4)
            assert sim.nbls_sim_fr_ntt(log2_n, direction, 4, pb, sb if shift else None, out, st) == 0
            return out.raw + st.raw
        return call

    def cells_mode():
        out, co, st = C.create_string_buffer(64 * n * 2), C.create_string_buffer(32 * n * 2), C.create_string_buffer(2)
        assert sim.nbls_sim_kzg_cells(log2_n, 2, rows(f) + rows(bad), out, co, st) == 0
        return out.raw + co.raw + st.raw
    zero = [0] * n
    for direction, ref in ((0, to_coeffs), (1, to_evals)):
        got = both_orders(sim, ntt(direction, True))
        assert ints(got[:-4]) == ref(f, log2_n, s) + zero + zero + zero and list(got[-4:]) == [0, 5, NON_CANONICAL, NON_CANONICAL]
        got = both_orders(sim, ntt(direction, False))
        assert ints(got[:-4]) == ref(f, log2_n) * 3 + zero and list(got[-4:]) == [0, 0, 0, NON_CANONICAL]
    got = both_orders(sim, cells_mode)
    assert ints(got[:64 * n]) == [v for cell in cells(f, log2_n, 0) for v in cell] and ints(got[64 * n:128 * n]) == zero * 2
    assert ints(got[128 * n:-2]) == to_coeffs(f, log2_n) + zero and list(got[-2:]) == [0, NON_CANONICAL]


# (1, 1) and (1, 0): the smallest shapes the launcher takes (M = 2: 256 stripes a workgroup, M = 4: 128; all but two resp. one past the call's last); (9, 0): one stripe a
# workgroup, two butterflies a lane; (4, 1) with 40 blobs: 80 stripes of M = 16 at 32 a workgroup -- three workgroups, the last one half empty
@pytest.mark.parametrize('log2_n,log2_cell,n', [(1, 1, 1), (1, 0, 1), (9, 0, 1), (4, 1, 40)])
def test_fk20_scalars(sim, log2_n, log2_cell, n):
    rnd = random.Random(9300 + 16 * log2_n + log2_cell)
    polys = [[rnd.randrange(R) for _ in range(1 << log2_n)] for _ in range(min(n, 3))]
    polys = [polys[i % len(polys)] for i in range(n)]
    pb = b''.join(rows(p) for p in polys)

    def call():
        out = C.create_string_buffer(32 * n * (2 << log2_n))
        assert sim.nbls_sim_kzg_fk20_scalars(log2_n, log2_cell, n, pb, out) == 0
        return out.raw
    want = {id(p): scalars_flat(p, log2_n, log2_cell) for p in polys[:3]}
    assert ints(both_orders(sim, call)) == [v for p in polys for v in want[id(p)]]


# (2, 0) and (2, 1): lanes idle in every phase; (10, 4): two elements a lane.  One call: a good blob, a refused index set, a non-canonical element, a contradiction
@pytest.mark.parametrize('log2_n,log2_cell', [(2, 0), (2, 1), (10, 4)])
def test_recovery(sim, log2_n, log2_cell):
    rnd = random.Random(9400 + 16 * log2_n + log2_cell)
    n, c, m = 1 << log2_n, 1 << log2_cell, n_cells(log2_n, log2_cell)
    coef = [rnd.randrange(R) for _ in range(n)]
    want = cells(to_evals(coef, log2_n), log2_n, log2_cell)
    half = rnd.sample(range(m), m // 2)
    more = half + [next(k for k in range(m) if k not in half)]
    take = lambda idx: [list(want[k]) for k in idx]
    non_canonical, contradiction = take(half), take(more)
    non_canonical[-1][c - 1] = R
    contradiction[0][0] = (contradiction[0][0] + 1) % R
    blobs = [(half, take(half)), (half[:-1], take(half[:-1])), (half, non_canonical), (more, contradiction), (more, take(more))]
    off = [0]
    for idx, _ in blobs:
        off.append(off[-1] + len(idx))
    flat = [k for idx, _ in blobs for k in idx]
    raw = b''.join(rows(cell) for _, given in blobs for cell in given)
    k = len(blobs)

    def call():
        out, co, st = C.create_string_buffer(64 * n * k), C.create_string_buffer(32 * n * k), C.create_string_buffer(k)
        assert sim.nbls_sim_kzg_recover(log2_n, log2_cell, k, (C.c_uint32 * (k + 1))(*off), (C.c_uint32 * len(flat))(*flat), raw, out, co, st) == 0
        return out.raw + co.raw + st.raw
    got = both_orders(sim, call)
    row, zero = [v for cell in want for v in cell], [0] * (2 * n)
    assert list(got[-k:]) == [0, BAD_CELLS, NON_CANONICAL, INCONSISTENT, 0]
    assert ints(got[:64 * n * k]) == row + zero * 3 + row
    assert ints(got[64 * n * k:-k]) == coef + [0] * (3 * n) + coef


# kzg_canon_kernel: one element a lane at most (log2_n = 1, 8) and two (9); a blob with its last element >= r between two good ones
@pytest.mark.parametrize('log2_n', [1, 8, 9])
def test_canonical_check(sim, log2_n):
    rnd = random.Random(9500 + log2_n)
    n = 1 << log2_n
    good = [rnd.randrange(R) for _ in range(n)]
    bad = good[:-1] + [R]

    def call():
        ev, st = C.create_string_buffer(rows(good) + rows(bad) + rows(good), 96 * n), C.create_string_buffer(3)
        assert sim.nbls_sim_kzg_canon(log2_n, 3, ev, st) == 0
        return ev.raw + st.raw
    got = both_orders(sim, call)
    assert ints(got[:-3]) == good + [0] * n + good and list(got[-3:]) == [0, NON_CANONICAL, 0]


# The three closing sums: a lane (kzg_sum_kernel), a lane group (kzg_cell_sum_kernel: 256 >> log2_cell groups) or a row group (g16_sum_kernel: sixteen) strides over the
# items; their number below, equal to and above the number of lanes or groups that stride -- none, one and two items for the last of them
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_sum_of_items(sim, n):
    rnd = random.Random(9600 + n)
    v = [rnd.choice([0, R - 1, rnd.randrange(R)]) for _ in range(n)]

    def call():
        out = C.create_string_buffer(32)
        assert sim.nbls_sim_kzg_sum(n, b''.join(map(b32, v)), out) == 0
        return out.raw
    assert ints(both_orders(sim, call)) == [-sum(v) % R]


@pytest.mark.parametrize('log2_cell,parts', [(0, 255), (0, 256), (0, 257), (6, 3), (6, 4), (6, 5)])
def test_sum_of_cell_rows(sim, log2_cell, parts):
    """`parts` workgroups of the interpolation leave as many partial rows for the closing kernel"""
    log2_n = 6
    rnd = random.Random(9700 + 16 * parts + log2_cell)
    c, m = 1 << log2_cell, 2 << (log2_n - log2_cell)
    n = (parts * 256 >> log2_cell) + 3          # every lane group of the launch has a cell, three have two
    kinds = [[rnd.randrange(R) for _ in range(c)] for _ in range(8)]
    pick = [(rnd.randrange(8), rnd.choice([0, 1, m // 2, m - 1]), rnd.randrange(1, R)) for _ in range(n)]          # (which cell, its index, its weight)
    cb, wb = b''.join(cell_bytes(kinds[j]) for j, _, _ in pick), b''.join(b32(w) for _, _, w in pick)

    def call():
        out = C.create_string_buffer(32 * c)
        assert sim.nbls_sim_kzg_cell_interp(log2_n, log2_cell, n, 1, parts, cb, (C.c_uint32 * n)(*[k for _, k, _ in pick]), None, wb, out, None) == 0
        return out.raw
    coeffs = {(j, k): interp_coeffs(kinds[j], k, log2_n, log2_cell) for j in range(8) for k in (0, 1, m // 2, m - 1)}
    want = [-sum(w * coeffs[j, k][i] for j, k, w in pick) % R for i in range(c)]          # kzg_verify_cells_cases.neg_sums, every cell interpolated once
    assert ints(both_orders(sim, call)) == want


@pytest.mark.parametrize('parts', [15, 16, 17])
@pytest.mark.parametrize('m', [3, 64])
def test_sum_of_groth16_rows(sim, m, parts):
    """`parts` workgroups of rows per tile leave as many partial rows; m = 64: two tiles, the second with one column"""
    rnd = random.Random(9800 + 100 * m + parts)
    n = parts * 16 + 5          # every row group of the launch has a row, five have two
    xs = [[rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(m)] for _ in range(n)]
    ws = [rnd.choice([1, (1 << 64) - 1, rnd.randrange(1 << 64)]) for _ in range(n)]
    xb, wb = b''.join(b32(x) for row in xs for x in row), b''.join(map(b32, ws))

    def call():
        out = C.create_string_buffer(32 * (m + 1))
        assert sim.nbls_sim_g16_input_sums(n, m, parts, xb, wb, None, out, None) == 0
        return out.raw
    assert ints(both_orders(sim, call)) == input_sums(xs, ws)[0]
