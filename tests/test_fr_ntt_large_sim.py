"""Transforms past one workgroup's LDS without a GPU: the bodies kzg_ntt_pass_kernel and kzg_ntt_tail_kernel compile for the device (fr_workgroup.h kzg_ntt_pass_body,
kzg_ntt_tail_body) on the simulator (nbls_sim_fr_ntt_large: launch after launch, one workgroup after another, 512 lanes each) against Python integers
(fr_ntt_large_cases.py, kzg_cells_cases.py) and against the one-workgroup transform (nbls_sim_fr_ntt).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256
from kzg_cells_cases import to_evals, to_coeffs, coset_shift, rows
from fr_ntt_large_cases import compose_to_evals, compose_to_coeffs

TO_COEFFS, TO_EVALS = 0, 1
NON_CANONICAL, ZERO_SHIFT = 21, 5
# (log2_n, tail bits, pass bits; 0 = the default)
PLANS = [(4, 2, 1), (6, 3, 1), (6, 3, 2), (6, 2, 4), (9, 4, 2), (13, 12, 0), (14, 12, 0), (15, 12, 1)]
SMALL = [p for p in PLANS if p[0] <= 12]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_fr_ntt_large.argtypes = [u, C.c_int, sz, vp, vp, vp, vp, u, u]
    lib.nbls_sim_fr_ntt.argtypes = [u, C.c_int, sz, vp, vp, vp, vp]
    lib.nbls_sim_set_lane_order.argtypes = [C.c_int]
    return lib


def large(sim, plan, direction, data, n, shifts=None, status=True):
    log2_n, t, p = plan
    out, st = C.create_string_buffer(max(len(data), 1)), C.create_string_buffer(b'\x7f' * max(n, 1), max(n, 1))
    assert sim.nbls_sim_fr_ntt_large(log2_n, direction, n, data, shifts, out, st if status else None, t, p) == 0
    return out.raw[:len(data)], list(st.raw[:n])


def small(sim, log2_n, direction, data, n, shifts=None):
    out, st = C.create_string_buffer(max(len(data), 1)), C.create_string_buffer(max(n, 1))
    assert sim.nbls_sim_fr_ntt(log2_n, direction, n, data, shifts, out, st) == 0
    return out.raw[:len(data)], list(st.raw[:n])


def reference(log2_n, t, direction, polys, shifts):
    """small sizes: the textbook network; above 2^12 the composition of fr_ntt_large_cases.py (its columns and tails are the textbook network)"""
    if log2_n <= 12:
        f = to_evals if direction == TO_EVALS else to_coeffs
        return [f(p, log2_n, s) for p, s in zip(polys, shifts)]
    f = compose_to_evals if direction == TO_EVALS else compose_to_coeffs
    return [f(p, log2_n, t, s) for p, s in zip(polys, shifts)]


def three(log2_n, seed):
    """n = 3: random, one row carrying 0 and r - 1 among random elements, random"""
    rnd, n = random.Random(seed), 1 << log2_n
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    polys[1][0], polys[1][n - 1], polys[1][n // 2] = 0, R - 1, R - 1
    polys[1][1] = 0
    return polys


@pytest.mark.parametrize('plan', PLANS, ids=str)
@pytest.mark.parametrize('direction', [TO_EVALS, TO_COEFFS])
def test_against_python(sim, plan, direction):
    log2_n, t, _ = plan
    polys = three(log2_n, 9000 + 100 * log2_n + t)
    data = b''.join(rows(p) for p in polys)
    rnd = random.Random(77)
    for shifts in (None, [rnd.randrange(1, R), 1, coset_shift(log2_n)]):
        want = reference(log2_n, t, direction, polys, shifts or [1, 1, 1])
        got, st = large(sim, plan, direction, data, 3, None if shifts is None else rows(shifts))
        assert st == [0, 0, 0]
        assert got == b''.join(rows(w) for w in want), ('shifts' if shifts else 'no shifts')


@pytest.mark.parametrize('plan', SMALL, ids=str)
def test_byte_equal_to_the_one_workgroup_transform(sim, plan):
    log2_n = plan[0]
    polys = three(log2_n, 9100 + log2_n)
    data, sh = b''.join(rows(p) for p in polys), rows([7, R - 1, 123456789])
    for direction in (TO_EVALS, TO_COEFFS):
        for shifts in (None, sh):
            assert large(sim, plan, direction, data, 3, shifts) == small(sim, log2_n, direction, data, 3, shifts)
    # status == NULL, and up to the tail size the call is the one-workgroup transform itself
    assert large(sim, plan, TO_EVALS, data, 3, sh, status=False)[0] == small(sim, log2_n, TO_EVALS, data, 3, sh)[0]
    assert large(sim, (log2_n, 12, 0), TO_EVALS, data, 3, sh) == small(sim, log2_n, TO_EVALS, data, 3, sh)


@pytest.mark.parametrize('plan', [(6, 2, 4), (9, 4, 2), (13, 12, 0)], ids=str)
def test_both_lane_orders_give_the_same_bytes(sim, plan):
    log2_n = plan[0]
    polys = three(log2_n, 9200 + log2_n)
    data, sh = b''.join(rows(p) for p in polys), rows([5, 0, R])          # one accepted, one zero shift, one shift >= r
    got = {}
    try:
        for order in (0, 1):
            sim.nbls_sim_set_lane_order(order)
            got[order] = [large(sim, plan, d, data, 3, sh) for d in (TO_EVALS, TO_COEFFS)]
    finally:
        sim.nbls_sim_set_lane_order(0)
    assert got[0] == got[1]
    assert got[0][0][1] == [0, ZERO_SHIFT, NON_CANONICAL]


@pytest.mark.parametrize('plan', [(4, 2, 1), (6, 3, 2), (9, 4, 2), (13, 12, 0)], ids=str)
@pytest.mark.parametrize('direction', [TO_EVALS, TO_COEFFS])
def test_refusals(sim, plan, direction):
    log2_n, t, _ = plan
    n, row = 1 << log2_n, 32 << log2_n
    polys = three(log2_n, 9300 + log2_n)
    good = b''.join(rows(p) for p in polys)
    shifts = [3, 11, coset_shift(log2_n)]
    clean, st = large(sim, plan, direction, good, 3, rows(shifts))
    assert st == [0, 0, 0]
    zero = bytes(row)
    # an element >= r in the LAST block of the middle polynomial: every other block of that row is accepted by the workgroup that reads it
    for bad_value in (R, M256):
        at = row + 32 * (n - 1 - (1 << t) // 2)
        data = good[:at] + bad_value.to_bytes(32, 'big') + good[at + 32:]
        got, st = large(sim, plan, direction, data, 3, rows(shifts))
        assert st == [0, NON_CANONICAL, 0]
        assert got[:row] == clean[:row] and got[row:2 * row] == zero and got[2 * row:] == clean[2 * row:]
    for bad_shift, code in ((R, NON_CANONICAL), (M256, NON_CANONICAL), (0, ZERO_SHIFT)):
        sh = rows([shifts[0]]) + bad_shift.to_bytes(32, 'big') + rows([shifts[2]])
        got, st = large(sim, plan, direction, good, 3, sh)
        assert st == [0, code, 0], bad_shift
        assert got[:row] == clean[:row] and got[row:2 * row] == zero and got[2 * row:] == clean[2 * row:]
    # non-canonical before zero: a zero shift on a row that also holds an element >= r
    data = good[:row] + R.to_bytes(32, 'big') + good[row + 32:]
    got, st = large(sim, plan, direction, data, 3, rows([shifts[0], 0, shifts[2]]))
    assert st == [0, NON_CANONICAL, 0] and got[row:2 * row] == zero


def test_in_place(sim):
    plan = (9, 4, 2)
    polys = three(9, 9400)
    data, sh = b''.join(rows(p) for p in polys), rows([7, 9, 11])
    for direction in (TO_EVALS, TO_COEFFS):
        want, _ = large(sim, plan, direction, data, 3, sh)
        buf, st = C.create_string_buffer(data, len(data)), C.create_string_buffer(3)
        assert sim.nbls_sim_fr_ntt_large(9, direction, 3, buf, sh, buf, st, 4, 2) == 0
        assert buf.raw == want and list(st.raw) == [0, 0, 0]


def test_argument_rules(sim):
    one, out = bytes(32 * 4), C.create_string_buffer(32 * 4)
    call = sim.nbls_sim_fr_ntt_large
    assert call(2, TO_EVALS, 1, one, None, out, None, 1, 1) == 0
    assert call(0, TO_EVALS, 1, one, None, out, None, 0, 0) == -1
    assert call(25, TO_EVALS, 1, one, None, out, None, 0, 0) == -1
    assert call(2, 2, 1, one, None, out, None, 0, 0) == -1
    assert call(2, -1, 1, one, None, out, None, 0, 0) == -1
    assert call(2, TO_EVALS, 1, None, None, out, None, 0, 0) == -1
    assert call(2, TO_EVALS, 1, one, None, None, None, 0, 0) == -1
    assert call(2, TO_EVALS, 0, None, None, None, None, 0, 0) == 0                      # n = 0
    assert call(2, TO_EVALS, (1 << 22) + 1, one, None, out, None, 0, 0) == -1           # more than 2^24 elements
    assert call(24, TO_EVALS, 2, one, None, out, None, 0, 0) == -1
    assert call(2, TO_EVALS, 1, one, None, out, None, 13, 0) == -1                      # the plan's ranges
    assert call(2, TO_EVALS, 1, one, None, out, None, 0, 10) == -1
    assert call(14, TO_EVALS, 1, one, None, out, None, 1, 0) == -1                      # more than 12 global stages
