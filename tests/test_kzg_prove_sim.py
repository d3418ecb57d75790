"""The quotient of an opening without a GPU: fr_eval_lane_t<true> / fr_quot_lane / fr_quot_within of fr_exec.h -- the code kzg_quotient_kernel compiles for the device -- on the
simulator (nbls_sim_fr_quotient_roots: 256 lanes per polynomial, the same terms per lane, the same two trees) against Python integers (kzg_prove_cases.quotient, the
within-domain formula taken literally from the EIP).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, LANES, NON_CANONICAL, b32, roots, eval_roots
from kzg_prove_cases import quotient, structured

SIZES = [1, 2, 6, 8, 9, 12]      # N = 2, 4, 64, 256, 512, 4096: below, at and above one term per lane


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_fr_quotient_roots.argtypes = [C.c_uint, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nbls_sim_fr_quotient_roots.restype = C.c_int
    return lib


def run(sim, log2_n, polys, zs, status=True):
    n, N = len(polys), 1 << log2_n
    y, q, st = C.create_string_buffer(max(32 * n, 1)), C.create_string_buffer(max(32 * n * N, 1)), C.create_string_buffer(max(n, 1))
    rc = sim.nbls_sim_fr_quotient_roots(log2_n, n, b''.join(b32(v) for f in polys for v in f), b''.join(map(b32, zs)), y, q, st if status else None)
    assert rc == 0
    ints = lambda raw, k: [int.from_bytes(raw[32 * i:32 * i + 32], 'big') for i in range(k)]
    qs = ints(q.raw, n * N)
    return ints(y.raw, n), [qs[i * N:(i + 1) * N] for i in range(n)], list(st.raw[:n])


@pytest.mark.parametrize('log2_n', SIZES)
def test_structured_cases_against_python(sim, log2_n):
    rnd = random.Random(2000 + log2_n)
    cases = structured(log2_n, rnd)
    ys, qs, st = run(sim, log2_n, [f for _, f, _ in cases], [z for _, _, z in cases])
    for (name, f, z), y, q, s in zip(cases, ys, qs, st):
        wy, wq = quotient(f, z, log2_n)
        assert s == 0, name
        assert y == wy == eval_roots(f, z, log2_n), name
        assert q == wq, name


@pytest.mark.parametrize('log2_n', SIZES)
def test_one_call_with_z_on_a_root_and_off_it(sim, log2_n):
    rnd = random.Random(2077 + log2_n)
    n, w = 1 << log2_n, roots(log2_n)
    f0, f1 = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]
    z1 = rnd.randrange(R)
    ys, qs, st = run(sim, log2_n, [f0, f1, f0], [w[n - 1], z1, w[1]])
    assert st == [0, 0, 0]
    for f, z, y, q in zip([f0, f1, f0], [w[n - 1], z1, w[1]], ys, qs):
        assert (y, q) == quotient(f, z, log2_n)
    ys2, qs2, _ = run(sim, log2_n, [f1, f0], [z1, w[1]], status=False)      # status == NULL
    assert (ys2, qs2) == ([ys[1], ys[2]], [qs[1], qs[2]])


def test_the_quotient_times_the_denominator_gives_back_the_polynomial(sim):
    """independent of both formulas: q(X) (X - z) = p(X) - y holds at every root, and where z = w_m the value q_m makes q a polynomial of degree < N - 1 (its values sum against
    the N-th Lagrange weights to a vanishing top coefficient: sum_j q_j w_j = 0 for N > 1)"""
    rnd = random.Random(2100)
    for log2_n in (2, 6):
        n, w = 1 << log2_n, roots(log2_n)
        f = [rnd.randrange(R) for _ in range(n)]
        for z in (rnd.randrange(R), w[3]):
            (y,), (q,), _ = run(sim, log2_n, [f], [z])
            for j in range(n):
                if w[j] != z:
                    assert q[j] * (w[j] - z) % R == (f[j] - y) % R
            assert sum(qj * wj for qj, wj in zip(q, w)) % R == 0      # the coefficient of X^(N-1) of q, times N


@pytest.mark.parametrize('log2_n', [2, 8, 9])
@pytest.mark.parametrize('bad', ['element=r', 'element=2^256-1', 'z=r'])
def test_non_canonical_inputs(sim, log2_n, bad):
    rnd = random.Random(2009 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [rnd.randrange(R), roots(log2_n)[n - 1], rnd.randrange(R)]
    want = [quotient(f, z, log2_n) for f, z in zip(fs, zs)]
    if bad == 'z=r':
        zs[1] = R
    else:
        fs[1] = list(fs[1])
        fs[1][n - 1 if log2_n != 9 else LANES + 3] = R if bad == 'element=r' else M256
    ys, qs, st = run(sim, log2_n, fs, zs)
    assert st == [0, NON_CANONICAL, 0]
    assert ys == [want[0][0], 0, want[2][0]]
    assert qs == [want[0][1], [0] * n, want[2][1]]
    assert run(sim, log2_n, fs, zs, status=False)[:2] == (ys, qs)


def test_argument_rules(sim):
    z = b32(1)
    y, q = C.create_string_buffer(64), C.create_string_buffer(32 * 8)
    assert sim.nbls_sim_fr_quotient_roots(0, 1, bytes(32), z, y, q, None) == -1
    assert sim.nbls_sim_fr_quotient_roots(13, 1, bytes(32), z, y, q, None) == -1
    assert sim.nbls_sim_fr_quotient_roots(2, 1, None, z, y, q, None) == -1
    assert sim.nbls_sim_fr_quotient_roots(2, 1, bytes(128), z, y, None, None) == -1
    assert sim.nbls_sim_fr_quotient_roots(12, 4097, None, None, None, None, None) == -1      # more than 2^24 elements
    assert sim.nbls_sim_fr_quotient_roots(2, 0, None, None, None, None, None) == 0
