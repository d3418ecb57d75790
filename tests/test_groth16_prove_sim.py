"""The Groth16 prover's scalar-field kernels without a GPU: the lane code the device compiles (g16p_exec.h) on the simulator -- nbls_sim_g16p_spmv (the witness check and the
three matrix-vector products, rows summed by a lane or by a wavefront), nbls_sim_g16p_quotient (the chain through the simulator's transforms) and nbls_sim_g16p_scalars --
against Python integers (groth16_prove_cases.py).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, b32
from groth16_prove_cases import instance, matvec, bitrev_order, quotient, csr, scalar_arrays, UNSATISFIED, NON_CANONICAL

# (log2_n, tail bits, pass bits; 0 = the default): 6 twice on the multi-pass route at a small size, 13 on the default plan
PLANS = [(1, 0, 0), (2, 0, 0), (4, 0, 0), (6, 3, 1), (6, 2, 4), (13, 0, 0)]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_g16p_spmv.argtypes = [u, sz, sz, vp, vp, u, vp, vp]
    lib.nbls_sim_g16p_quotient.argtypes = [u, sz, vp, vp, vp, vp, vp, u, u]
    lib.nbls_sim_g16p_scalars.argtypes = [u, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nbls_sim_set_lane_order.argtypes = [C.c_int]
    return lib


def pack(v):
    return b''.join(b32(x) for x in v)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 32], 'big') for i in range(0, len(raw), 32)]


def spmv(sim, log2_n, mats, z, r=3, s=4, row_wave=0):
    """-> (a, b, c as ints in bit-reversed order, (non-canonical, unsatisfied))"""
    keep, ptrs = [], (C.c_void_p * 9)()
    for k, M in enumerate(mats):
        offs, cols, vals = csr(M)
        bufs = ((C.c_uint32 * len(offs))(*offs), (C.c_uint32 * max(len(cols), 1))(*cols), C.create_string_buffer(vals, max(len(vals), 1)))
        keep.append(bufs)
        for f, b in enumerate(bufs):
            ptrs[3 * k + f] = C.cast(b, C.c_void_p)
    N = 1 << log2_n
    out, flags = C.create_string_buffer(b'\x55' * (96 * N), 96 * N), C.create_string_buffer(b'\x7f\x7f', 2)
    assert sim.nbls_sim_g16p_spmv(log2_n, len(z), len(mats[0]), ptrs, pack(z + [r, s]), row_wave, out, flags) == 0
    v = unpack(out.raw[:96 * N])
    return v[:N], v[N:2 * N], v[2 * N:], tuple(flags.raw[:2])


def expected(mats, z, log2_n):
    return tuple(bitrev_order(matvec(M, [x % R for x in z], log2_n), log2_n) for M in mats)


@pytest.fixture(scope='module')
def ragged():
    """rows of 0, 1, 63, 64, 65 and n_vars entries among short ones; column 5 named by no row; z holds 0 and r - 1"""
    rnd, log2_n, n_vars = random.Random(1701), 5, 80
    z = [1, 0, R - 1] + [rnd.randrange(R) for _ in range(n_vars - 3)]
    lengths = [(0, 0), (1, 1), (63, 2), (2, 64), (65, 65), (n_vars - 1, n_vars - 1), (0, 3), (64, 0)] + [(rnd.randrange(1, 4), rnd.randrange(1, 4)) for _ in range(18)]
    A, B, Cm, z = instance(log2_n, n_vars, 3, rnd, lengths=lengths, z=z, skip=(5,))
    assert not any(c == 5 for M in (A, B, Cm) for row in M for c, _ in row)
    return log2_n, (A, B, Cm), z


@pytest.mark.parametrize('row_wave', [1, 8, 64, 0])
def test_products_by_lane_and_by_wavefront(sim, ragged, row_wave):
    log2_n, mats, z = ragged
    a, b, c, flags = spmv(sim, log2_n, mats, z, row_wave=row_wave)
    assert (a, b, c) == expected(mats, z, log2_n) and flags == (0, 0)


def test_every_column_named(sim):
    """rows that name all n_vars columns"""
    rnd, log2_n, n_vars = random.Random(1702), 2, 70
    mats = instance(log2_n, n_vars, 1, rnd, lengths=[(n_vars, n_vars), (1, n_vars), (n_vars, 1)])
    z = mats[3]
    for row_wave in (1, 0, 70, 71):
        a, b, c, flags = spmv(sim, log2_n, mats[:3], z, row_wave=row_wave)
        assert (a, b, c) == expected(mats[:3], z, log2_n) and flags == (0, 0)


@pytest.mark.parametrize('log2_n', [1, 2, 4, 6])
def test_products_at_small_sizes(sim, log2_n):
    rnd = random.Random(1710 + log2_n)
    A, B, Cm, z = instance(log2_n, 12, 2, rnd)
    a, b, c, flags = spmv(sim, log2_n, (A, B, Cm), z)
    assert (a, b, c) == expected((A, B, Cm), z, log2_n) and flags == (0, 0)
    assert all(x == 0 for x in bitrev_order(a, log2_n)[len(A):])          # the rows past the last constraint are written, as zeros


def test_flags(sim, ragged):
    log2_n, mats, z = ragged
    A, B, Cm = mats
    # one violated row, a short one and the longest
    for j in (1, 5):
        k, v = Cm[j][0]
        spoiled = Cm[:j] + [[(k, (v + 1) % R)]] + Cm[j + 1:]
        for row_wave in (1, 0):
            a, b, c, flags = spmv(sim, log2_n, (A, B, spoiled), z, row_wave=row_wave)
            assert flags == (0, 1) and (a, b, c) == expected((A, B, spoiled), z, log2_n)
    # z_0 = 2: every product is what the matrices give, and the flag is raised for z_0 alone where no row names column 0 ...
    rnd = random.Random(1703)
    A2, B2, C2, z2 = instance(3, 9, 2, rnd, skip=(0,))
    assert spmv(sim, 3, (A2, B2, C2), z2)[3] == (0, 0)
    assert spmv(sim, 3, (A2, B2, C2), [2] + z2[1:])[3] == (0, 1)
    assert spmv(sim, 3, (A2, B2, C2), [0] + z2[1:])[3] == (0, 1)
    # an element = r, in z, in r, in s: non-canonical (z_0 = r + 1 is both)
    assert spmv(sim, 3, (A2, B2, C2), z2[:4] + [R] + z2[5:])[3][0] == 1
    assert spmv(sim, 3, (A2, B2, C2), z2, r=R)[3] == (1, 0)
    assert spmv(sim, 3, (A2, B2, C2), z2, s=M256)[3] == (1, 0)
    assert spmv(sim, 3, (A2, B2, C2), [R + 1] + z2[1:])[3] == (1, 1)
    assert spmv(sim, 3, (A2, B2, C2), z2, r=R - 1, s=0)[3] == (0, 0)


def test_matrix_rules(sim):
    rnd = random.Random(1704)
    A, B, Cm, z = instance(2, 6, 1, rnd)
    ptrs = (C.c_void_p * 9)()
    out, flags = C.create_string_buffer(96 * 4), C.create_string_buffer(2)

    def call(offs, cols, vals, n_cons=3, log2_n=2):
        bufs = ((C.c_uint32 * len(offs))(*offs), (C.c_uint32 * max(len(cols), 1))(*cols), C.create_string_buffer(vals, max(len(vals), 1)))
        for k in range(3):
            for f, b in enumerate(bufs):
                ptrs[3 * k + f] = C.cast(b, C.c_void_p)
        return sim.nbls_sim_g16p_spmv(log2_n, 6, n_cons, ptrs, pack(z + [1, 1]), 0, out, flags)

    offs, cols, vals = csr(A)
    assert call(offs, cols, vals) == 0
    assert call([1] + offs[1:], cols, vals) == -1                      # offsets that do not start at 0
    assert offs[1] < offs[2] and call([0, offs[2], offs[1], offs[3]], cols, vals) == -1          # decreasing offsets
    assert call(offs, [6] + cols[1:], vals) == -1                      # a column >= n_vars
    assert call(offs, cols, b32(R) + vals[32:]) == -1                  # a non-canonical coefficient
    assert call(offs, cols, vals, n_cons=5) == -1                      # more constraints than N
    assert call(offs, cols, vals, log2_n=0) == -1 and call(offs, cols, vals, log2_n=22) == -1


def run_quotient(sim, plan, a, b, c, status=True):
    log2_n, t, p = plan
    n = len(a)
    out, st = C.create_string_buffer(b'\x55' * (n * 32 << log2_n), n * 32 << log2_n), C.create_string_buffer(b'\x7f' * n, n)
    assert sim.nbls_sim_g16p_quotient(log2_n, n, pack(sum(a, [])), pack(sum(b, [])), pack(sum(c, [])), out, st if status else None, t, p) == 0
    N = 1 << log2_n
    h = unpack(out.raw[:n * 32 * N])
    return [h[i * N:i * N + N] for i in range(n)], list(st.raw[:n])


def triples(log2_n, seed):
    """three satisfied triples; the middle one carries 0 and r - 1"""
    rnd, N = random.Random(seed), 1 << log2_n
    a = [[rnd.randrange(R) for _ in range(N)] for _ in range(3)]
    b = [[rnd.randrange(R) for _ in range(N)] for _ in range(3)]
    a[1][0], a[1][N - 1], b[1][N - 1], b[1][N // 2] = 0, R - 1, R - 1, 0
    return a, b, [[x * y % R for x, y in zip(ra, rb)] for ra, rb in zip(a, b)]


@pytest.mark.parametrize('plan', PLANS, ids=str)
def test_quotient(sim, plan):
    log2_n = plan[0]
    a, b, c = triples(log2_n, 1720 + log2_n)
    h, st = run_quotient(sim, plan, a, b, c)
    assert st == [0, 0, 0]
    for i in range(3 if log2_n < 13 else 1):          # (one row of 2^13 in Python integers is enough: the three share every launch)
        assert h[i] == quotient(a[i], b[i], c[i], log2_n) and h[i][-1] == 0


@pytest.mark.parametrize('plan', [(2, 0, 0), (6, 3, 1)], ids=str)
def test_quotient_statuses(sim, plan):
    log2_n = plan[0]
    a, b, c = triples(log2_n, 1730 + log2_n)
    good, _ = run_quotient(sim, plan, a, b, c)
    # a violated row, an element = r (in a, b or c), both: the neighbours' bytes do not change
    for which in range(3):
        bad = [[row[:] for row in v] for v in (a, b, c)]
        bad[which][1][3] = R
        h, st = run_quotient(sim, plan, *bad)
        assert st == [0, NON_CANONICAL, 0] and h[1] == [0] * (1 << log2_n) and h[0] == good[0] and h[2] == good[2]
    c2 = [row[:] for row in c]
    c2[2][1] = (c2[2][1] + 1) % R
    h, st = run_quotient(sim, plan, a, b, c2)
    assert st == [0, 0, UNSATISFIED] and h[:2] == good[:2]
    c2[2][0] = M256
    h, st = run_quotient(sim, plan, a, b, c2)
    assert st == [0, 0, NON_CANONICAL] and h[2] == [0] * (1 << log2_n) and h[:2] == good[:2]
    assert run_quotient(sim, plan, a, b, c, status=False)[0] == good


def test_quotient_refusals(sim):
    x = b32(1) * 4
    out = C.create_string_buffer(128)
    assert sim.nbls_sim_g16p_quotient(0, 1, x, x, x, out, None, 0, 0) == -1
    assert sim.nbls_sim_g16p_quotient(23, 1, x, x, x, out, None, 0, 0) == -1
    assert sim.nbls_sim_g16p_quotient(14, 1, x, x, x, out, None, 1, 0) == -1          # more than 12 global stages
    assert sim.nbls_sim_g16p_quotient(2, 1, None, x, x, out, None, 0, 0) == -1
    assert sim.nbls_sim_g16p_quotient(2, 1, x, x, x, None, None, 0, 0) == -1
    assert sim.nbls_sim_g16p_quotient(12, 4097, x, x, x, out, None, 0, 0) == -1
    assert sim.nbls_sim_g16p_quotient(2, 0, None, None, None, None, None, 0, 0) == 0
    assert out.raw == bytes(128)


def run_scalars(sim, log2_n, m, z, r, s, h, masks, flags=(0, 0)):
    n_vars, N = len(z), 1 << log2_n
    na = n_vars - m - 1
    sa, sb, sc = C.create_string_buffer(32 * (n_vars + 2)), C.create_string_buffer(32 * (n_vars + 2)), C.create_string_buffer(32 * (na + N + 2))
    ma, mb, ml = (bytes(bytearray(k)) for k in masks)
    assert sim.nbls_sim_g16p_scalars(log2_n, n_vars, m, pack(z + [r, s]), pack(h), ma, mb, ml if na else None, bytes(bytearray(flags)), sa, sb, sc) == 0
    return unpack(sa.raw), unpack(sb.raw), unpack(sc.raw)


@pytest.mark.parametrize('shape', [(1, 4, 1), (2, 3, 2), (4, 20, 3), (6, 70, 4)], ids=str)
def test_scalars(sim, shape):
    log2_n, n_vars, m = shape
    rnd, N = random.Random(1740 + log2_n), 1 << log2_n
    z = [1] + [rnd.randrange(R) for _ in range(n_vars - 1)]
    h = [rnd.randrange(R) for _ in range(N - 1)] + [0]
    r, s = rnd.randrange(R), rnd.randrange(R)
    na = n_vars - m - 1
    masks = ([rnd.randrange(4) == 0 for _ in range(n_vars)], [rnd.randrange(3) == 0 for _ in range(n_vars)], [rnd.randrange(2) == 0 for _ in range(na)])
    none = ([0] * n_vars, [0] * n_vars, [0] * na)
    for mk in (none, masks):
        assert run_scalars(sim, log2_n, m, z, r, s, h, mk) == scalar_arrays(z, r, s, h, m, *mk)
    assert run_scalars(sim, log2_n, m, z, R - 1, R - 1, h, none) == scalar_arrays(z, R - 1, R - 1, h, m, *none)
    assert run_scalars(sim, log2_n, m, z, 0, s, h, none)[2][-1] == 0
    # a refused witness: every scalar zero, whatever it holds
    for flags in ((1, 0), (0, 1), (1, 1)):
        assert run_scalars(sim, log2_n, m, [R] + z[1:], M256, s, h, masks, flags) == scalar_arrays(z, r, s, h, m, *masks, dead=True)


def test_lane_order_does_not_change_a_byte(sim, ragged):
    log2_n, mats, z = ragged
    a, b, c = triples(6, 1750)
    rnd = random.Random(1751)
    h = [rnd.randrange(R) for _ in range(31)] + [0]
    masks = ([0] * len(z), [i % 3 == 0 for i in range(len(z))], [0] * (len(z) - 4))
    up = [spmv(sim, log2_n, mats, z, row_wave=w) for w in (1, 8, 0)], run_quotient(sim, (6, 3, 1), a, b, c), run_scalars(sim, log2_n, 3, z, 5, 6, h, masks)
    sim.nbls_sim_set_lane_order(1)
    try:
        down = [spmv(sim, log2_n, mats, z, row_wave=w) for w in (1, 8, 0)], run_quotient(sim, (6, 3, 1), a, b, c), run_scalars(sim, log2_n, 3, z, 5, 6, h, masks)
    finally:
        sim.nbls_sim_set_lane_order(0)
    assert up == down
