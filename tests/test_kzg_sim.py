"""Polynomials in evaluation form without a GPU: fr_eval_lane / fr_eval_finish of fr_exec.h -- the code kzg_kernels.hip compiles for the device -- on the simulator
(nbls_sim_fr_eval_roots: 256 lanes per polynomial, the same terms per lane, the same tree of additions) against Python integers (kzg_cases.py).  Bit-exact."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R, M256, LANES, NON_CANONICAL, b32, roots, eval_roots, horner, evals_of

SIZES = [1, 2, 6, 8, 9, 12]      # N = 2, 4, 64, 256, 512, 4096: below, at and above one term per lane


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_fr_eval_roots.argtypes = [C.c_uint, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nbls_sim_fr_eval_roots.restype = C.c_int
    return lib


def run(sim, log2_n, polys, zs, status=True):
    n = len(polys)
    out, st = C.create_string_buffer(max(32 * n, 1)), C.create_string_buffer(max(n, 1))
    rc = sim.nbls_sim_fr_eval_roots(log2_n, n, b''.join(b32(v) for f in polys for v in f), b''.join(map(b32, zs)), out, st if status else None)
    assert rc == 0
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], 'big') for i in range(n)], list(st.raw[:n])


def structured(log2_n, rnd):
    """(name, f, z) for every polynomial and evaluation point the issue lists, at N = 2^log2_n"""
    n, w = 1 << log2_n, roots(log2_n)
    polys = {'random': [rnd.randrange(R) for _ in range(n)], 'zero': [0] * n, 'constant': [rnd.randrange(1, R)] * n, 'X': list(w),
             'r-1': [R - 1 if j == n // 2 else rnd.randrange(R) for j in range(n)]}
    # z on a root: the first and the last term, and one term on each side of where a lane's range ends (lane 255 -> lane 0's next term; the last term of lane 0 and the first of lane 1)
    on = sorted({0, n - 1, min(LANES - 1, n - 1), min(LANES, n - 1), max(n - LANES, 0), min(n - LANES + 1, n - 1) if n > LANES else 1})
    points = [('random', rnd.randrange(R)), ('0', 0), ('r-1', R - 1)] + [('w%d' % j, w[j]) for j in on]
    return [(pn + '@' + zn, f, z) for pn, f in polys.items() for zn, z in points]


@pytest.mark.parametrize('log2_n', SIZES)
@pytest.mark.parametrize('n', [1, 3])
def test_structured_cases_against_python(sim, log2_n, n):
    rnd = random.Random(1000 * log2_n + n)
    cases = structured(log2_n, rnd)
    for k in range(0, len(cases), n):
        part = cases[k:k + n]
        got, st = run(sim, log2_n, [f for _, f, _ in part], [z for _, _, z in part])
        for (name, f, z), g, s in zip(part, got, st):
            assert s == 0, name
            assert g == eval_roots(f, z, log2_n), name


@pytest.mark.parametrize('log2_n', SIZES)
def test_one_call_with_z_on_a_root_and_off_it(sim, log2_n):
    rnd = random.Random(77 + log2_n)
    n, w = 1 << log2_n, roots(log2_n)
    f0, f1 = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]
    z1 = rnd.randrange(R)
    got, st = run(sim, log2_n, [f0, f1], [w[n - 1], z1])
    assert st == [0, 0]
    assert got == [f0[n - 1], eval_roots(f1, z1, log2_n)]
    got, st = run(sim, log2_n, [f1, f0], [z1, w[1]], status=False)      # status == NULL
    assert got == [eval_roots(f1, z1, log2_n), f0[1]]


@pytest.mark.parametrize('log2_n', [1, 2, 6])
def test_against_horner_on_a_coefficient_form_polynomial(sim, log2_n):
    """independent of the barycentric formula: the values of a polynomial of degree < N on the roots determine it"""
    rnd = random.Random(5 + log2_n)
    n = 1 << log2_n
    for deg in sorted({0, 1, n // 2, n - 1}):
        coef = [rnd.randrange(R) for _ in range(deg + 1)]
        zs = [rnd.randrange(R), 0, R - 1, roots(log2_n)[n - 1]]
        got, st = run(sim, log2_n, [evals_of(coef, log2_n)] * len(zs), zs)
        assert st == [0] * len(zs)
        assert got == [horner(coef, z) for z in zs], deg


@pytest.mark.parametrize('log2_n', [2, 8, 9])
@pytest.mark.parametrize('bad', ['element=r', 'element=2^256-1', 'z=r'])
def test_non_canonical_inputs(sim, log2_n, bad):
    rnd = random.Random(9 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [rnd.randrange(R) for _ in range(3)]
    want = [eval_roots(f, z, log2_n) for f, z in zip(fs, zs)]
    if bad == 'z=r':
        zs[1] = R
    else:
        fs[1] = list(fs[1])
        fs[1][n - 1 if log2_n != 9 else LANES + 3] = R if bad == 'element=r' else M256
    got, st = run(sim, log2_n, fs, zs)
    assert st == [0, NON_CANONICAL, 0]
    assert got == [want[0], 0, want[2]]


def test_argument_rules(sim):
    z = b32(1)
    out, st = C.create_string_buffer(64), C.create_string_buffer(2)
    assert sim.nbls_sim_fr_eval_roots(0, 1, bytes(32), z, out, st) == -1
    assert sim.nbls_sim_fr_eval_roots(13, 1, bytes(32 * 8192), z, out, st) == -1
    assert sim.nbls_sim_fr_eval_roots(2, 1, None, z, out, st) == -1
    assert sim.nbls_sim_fr_eval_roots(12, 4097, None, None, None, None) == -1      # more than 2^24 elements
    assert sim.nbls_sim_fr_eval_roots(2, 0, None, None, None, None) == 0
