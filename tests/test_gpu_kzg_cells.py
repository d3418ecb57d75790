"""PeerDAS on the GPU (-m gpu): nbls_fr_ntt, nbls_kzg_compute_cells and nbls_kzg_compute_cells_and_proofs against Python integers (kzg_cells_cases.py) and kzg_cases.py's
test-only trusted setup: with tau known a cell's proof is [q_k(tau)]G1, one multiple of the generator from the oracle, so equality with the device's bytes is exact.  Nothing
expected comes from the calls under test; what they produce is then fed to the existing verifier and compared with the existing prover.

The transform kernel has 512 lanes per polynomial: up to N = 512 a lane owns at most one element and one butterfly per stage, at N = 1024 two elements and one butterfly, at
2048 four and two, at 4096 eight and four -- hence the sizes 10 and 11 beside the issue's 1, 2, 8, 9, 12."""
import ctypes as C
import importlib
import random
import pytest
from goldenio import hx
from kzg_cases import R, M256, NON_CANONICAL, ZERO48, Setup, b32, roots, horner, blob_bytes
from kzg_prove_cases import lagrange_setup
from kzg_cells_cases import LANES, to_evals, to_coeffs, coset_shift, cells, cell_points, cell_proof, monomial_setup, structured

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
EINVAL, EDECODE, ZERO_SHIFT = -1, -5, 5


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


@pytest.fixture(scope='module')
def setup(eng, oracle):
    return Setup(oracle, eng)


@pytest.fixture(scope='module')
def mono(eng, setup):
    """log2_n -> the device-resident monomial basis of that size, created on first use"""
    made = {}

    def get(log2_n):
        if log2_n not in made:
            made[log2_n] = eng.kzg_monomial_setup(log2_n, monomial_setup(setup, log2_n))
        return made[log2_n]
    yield get
    for s in made.values():
        s.close()


def ints(vals):
    return [int.from_bytes(v, 'big') for v in vals]


def cell_ints(cell_rows):
    """the cells of one blob as the engine returns them -> lists of integers"""
    return [[int.from_bytes(c[32 * j:32 * j + 32], 'big') for j in range(len(c) // 32)] for c in cell_rows]


# ---- (a) nbls_fr_ntt

@pytest.mark.parametrize('log2_n', [1, 2, 8, 9, 10, 11, 12])
def test_ntt_structured_cases(eng, log2_n):
    rnd = random.Random(600 + log2_n)
    cases = structured(log2_n, rnd)
    polys = [f for _, f in cases]
    kinds = [1, coset_shift(log2_n), R - 1, rnd.randrange(1, R)]
    for sh in [None] + [[s] * len(polys) for s in kinds]:
        for to_ev, ref in ((True, to_evals), (False, to_coeffs)):
            got, st = eng.fr_ntt(log2_n, polys, to_ev, sh)
            assert st == [0] * len(polys)
            for i, (name, f) in enumerate(cases):
                assert ints(got[i]) == ref(f, log2_n, 1 if sh is None else sh[i]), (name, to_ev, None if sh is None else sh[i])


@pytest.mark.parametrize('log2_n', [2, 9, 12])
def test_ntt_one_polynomial_and_five(eng, log2_n):
    rnd = random.Random(620 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
    ss = [rnd.randrange(1, R), 1, coset_shift(log2_n), R - 1, rnd.randrange(1, R)]
    for to_ev, ref in ((True, to_evals), (False, to_coeffs)):
        got, st = eng.fr_ntt(log2_n, fs[:1], to_ev)
        assert st == [0] and ints(got[0]) == ref(fs[0], log2_n)
        got, st = eng.fr_ntt(log2_n, fs, to_ev, ss)
        assert st == [0] * 5 and [ints(g) for g in got] == [ref(f, log2_n, s) for f, s in zip(fs, ss)]
    coef, _ = eng.fr_ntt(log2_n, fs, False, ss)
    back, _ = eng.fr_ntt(log2_n, [ints(c) for c in coef], True, ss)
    assert [ints(b) for b in back] == fs          # the round trip


@pytest.mark.parametrize('log2_n', [2, 9, 12])
def test_ntt_against_the_barycentric_evaluation_on_the_device(eng, log2_n):
    rnd = random.Random(640 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [rnd.randrange(R), roots(log2_n)[n - 1], 0]
    coef, st = eng.fr_ntt(log2_n, fs, False)
    ys, st2 = eng.fr_eval_roots(log2_n, fs, zs)
    assert st == [0, 0, 0] and st2 == [0, 0, 0]
    assert [horner(ints(c), z) for c, z in zip(coef, zs)] == ints(ys)


def test_ntt_refused_inputs_and_return_codes(eng):
    rnd = random.Random(660)
    for log2_n in (2, 10):
        n = 1 << log2_n
        fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
        ss = [rnd.randrange(1, R) for _ in range(5)]
        for to_ev, ref in ((True, to_evals), (False, to_coeffs)):
            want = [ref(f, log2_n, s) for f, s in zip(fs, ss)]
            polys, sh = [list(f) for f in fs], list(ss)
            polys[1][n - 1 if log2_n == 2 else LANES + 3] = R
            polys[3][0] = M256
            got, st = eng.fr_ntt(log2_n, polys, to_ev, sh)
            assert st == [0, NON_CANONICAL, 0, NON_CANONICAL, 0]
            assert [ints(g) for g in got] == [want[0], [0] * n, want[2], [0] * n, want[4]]
            sh[0], sh[2] = R, 0
            got, st = eng.fr_ntt(log2_n, fs, to_ev, sh)
            assert st == [NON_CANONICAL, 0, ZERO_SHIFT, 0, 0]
            assert [ints(g) for g in got] == [[0] * n, want[1], [0] * n, want[3], want[4]]
    lib, x, out = eng.lib, bytes(128), C.create_string_buffer(128)
    assert lib.nbls_fr_ntt(eng.h, 2, 0, 0, None, None, None, None) == 0
    assert lib.nbls_fr_ntt(eng.h, 2, 2, 1, x, None, out, None) == EINVAL
    assert lib.nbls_fr_ntt(eng.h, 13, 0, 1, x, None, out, None) == EINVAL
    assert lib.nbls_fr_ntt(eng.h, 2, 1, 1, x, None, out, None) == 0 and out.raw == bytes(128)          # status == NULL; the zero polynomial


# ---- (b) nbls_kzg_compute_cells

@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (2, 1), (6, 0), (5, 5), (8, 3), (9, 6), (12, 6)])
def test_compute_cells(eng, log2_n, log2_cell):
    rnd = random.Random(700 + 16 * log2_n + log2_cell)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    blobs = [blob_bytes(f) for f in fs]
    raw = bytearray(blobs[1]); raw[32 * (n // 2):32 * (n // 2) + 32] = b32(R); blobs[1] = bytes(raw)          # a refused blob between two good ones
    got, st = eng.kzg_compute_cells(log2_n, log2_cell, blobs)
    assert st == bytes([0, NON_CANONICAL, 0])
    per, cell = 2 << (log2_n - log2_cell), 32 << log2_cell
    assert [len(g) for g in got] == [per] * 3 and got[1] == [bytes(cell)] * per
    for i in (0, 2):
        assert b''.join(got[i][:per // 2]) == blobs[i]          # the first half is the blob
        assert cell_ints(got[i]) == cells(fs[i], log2_n, log2_cell)
    alone, st = eng.kzg_compute_cells(log2_n, log2_cell, blobs[2:])
    assert (alone, st) == ([got[2]], bytes(1))


# ---- (c) the monomial basis

def test_monomial_setup_reports_its_size_and_refuses_bad_entries(pkg, eng, setup, mono, golden):
    assert mono(2).log2_n == 2 and mono(6).log2_n == 6
    vec = golden['codec']['g1']
    bad = {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}
    good = monomial_setup(setup, 2)
    for name, want in (('subgroup', 3), ('noroot', 4)):
        pts = list(good); pts[2] = bad[name]
        with pytest.raises(pkg.KzgSetupError) as e:
            eng.kzg_monomial_setup(2, pts)
        assert (e.value.code, e.value.status) == (EDECODE, bytes([0, 0, want, 0])), name
    pts = list(good); pts[1] = ZERO48
    with pytest.raises(pkg.KzgSetupError) as e:
        eng.kzg_monomial_setup(2, pts)
    assert (e.value.code, e.value.status) == (EDECODE, bytes([0, 1, 0, 0]))
    out = C.c_void_p(7)
    assert eng.lib.nbls_kzg_monomial_create(eng.h, 2, b''.join(pts), None, C.byref(out)) == EDECODE and out.value is None
    assert eng.lib.nbls_kzg_monomial_create(eng.h, 13, b''.join(pts), None, C.byref(out)) == EINVAL


# ---- (d) nbls_kzg_compute_cells_and_proofs

def proof_blobs(log2_n, log2_cell, rnd):
    """name -> (blob values, coefficients): a random polynomial, the zero polynomial, a polynomial of degree < c and, where c < N, X^c"""
    n, c = 1 << log2_n, 1 << log2_cell
    coefs = {'random': [rnd.randrange(R) for _ in range(n)], 'zero': [0] * n, 'degree<c': [rnd.randrange(1, R) for _ in range(c)] + [0] * (n - c)}
    if c < n:
        coefs['X^c'] = [0] * c + [1] + [0] * (n - c - 1)
    return {k: (to_evals(v, log2_n), v) for k, v in coefs.items()}


@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (6, 0), (5, 5), (8, 3)])
def test_cells_and_proofs(eng, setup, mono, log2_n, log2_cell):
    rnd = random.Random(800 + 16 * log2_n + log2_cell)
    cases = proof_blobs(log2_n, log2_cell, rnd)
    per = 2 << (log2_n - log2_cell)
    got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs(mono(log2_n), log2_cell, [blob_bytes(f) for f, _ in cases.values()])
    assert st == bytes(len(cases))
    assert (got_cells, bytes(len(cases))) == eng.kzg_compute_cells(log2_n, log2_cell, [blob_bytes(f) for f, _ in cases.values()])
    for (name, (f, coef)), cs, ps in zip(cases.items(), got_cells, got_proofs):
        assert cell_ints(cs) == cells(f, log2_n, log2_cell), name
        assert ps == [cell_proof(setup, coef, k, log2_n, log2_cell) for k in range(per)], name
        if name in ('zero', 'degree<c'):
            assert ps == [ZERO48] * per, name          # the quotient is zero: the zero point, status 0
        if name == 'X^c':
            assert ps == [setup.g1(1)] * per          # X^c = 1 * (X^c - s_k) + s_k: every quotient is 1
    if log2_cell == log2_n:
        assert all(len(ps) == 2 and ps == [ZERO48] * 2 for ps in got_proofs)


def test_mainnet_size(eng, setup, mono):
    rnd = random.Random(880)
    f = [rnd.randrange(R) for _ in range(4096)]
    coef = to_coeffs(f, 12)
    got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs(mono(12), 6, [blob_bytes(f)])
    assert st == bytes(1) and cell_ints(got_cells[0]) == cells(f, 12, 6)
    assert got_proofs[0] == [cell_proof(setup, coef, k, 12, 6) for k in range(128)]          # every cell: 128 quotients and as many oracle multiplications


def test_single_element_cells_against_the_verifier_and_the_prover(eng, setup, mono):
    """log2_cell = 0: a cell is one value y = p(z) at the point z = h_k and its proof is the opening proof at z.  The existing verifier accepts every one of them, and for the
    cells of the blob itself (k < N, z = w_k) the bytes are those of nbls_kzg_compute_proofs"""
    rnd = random.Random(890)
    f = [rnd.randrange(R) for _ in range(64)]
    blob = blob_bytes(f)
    got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs(mono(6), 0, [blob])
    zs = [cell_points(k, 6, 0)[0] for k in range(128)]
    ys = [c[0] for c in cell_ints(got_cells[0])]
    assert st == bytes(1) and zs[:64] == roots(6)
    assert eng.kzg_verify_proofs([setup.commit(f, 6)] * 128, zs, ys, got_proofs[0], setup.tau_g2(), seed=SEED) == (True, bytes(128))
    lag = eng.kzg_setup(6, lagrange_setup(setup, 6))
    ps, py, pst = eng.kzg_compute_proofs(lag, [blob] * 64, zs[:64])
    lag.close()
    assert (ps, ints(py), pst) == (got_proofs[0][:64], f, bytes(64))


def test_chunks_give_the_same_bytes(pkg, setup, mono):
    rnd = random.Random(895)
    blobs = [blob_bytes([rnd.randrange(R) for _ in range(32)]) for _ in range(3)]
    other = pkg.Engine(0)
    runs = []
    for chunk in (1, 2, 0):
        other.set_cells_chunk(chunk)
        runs.append(other.kzg_compute_cells_and_proofs(mono(5), 2, blobs))
    assert other.lib.nbls_set_tuning(other.h, 20, -1) == EINVAL
    other.close()
    assert runs[0] == runs[1] == runs[2] and runs[0][2] == bytes(3)
    coef = to_coeffs([int.from_bytes(blobs[2][32 * j:32 * j + 32], 'big') for j in range(32)], 5)
    assert runs[0][1][2] == [cell_proof(setup, coef, k, 5, 2) for k in range(16)]          # the last blob: alone in its pass with chunks of one and of two


def test_a_refused_blob_between_two_good_ones(eng, setup, mono):
    rnd = random.Random(897)
    fs = [[rnd.randrange(R) for _ in range(32)] for _ in range(3)]
    blobs = [blob_bytes(f) for f in fs]
    raw = bytearray(blobs[1]); raw[32 * 31:] = b32(M256); blobs[1] = bytes(raw)
    for chunk in (0, 1):
        eng.set_cells_chunk(chunk)
        got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs(mono(5), 2, blobs)
        assert st == bytes([0, NON_CANONICAL, 0])
        assert got_cells[1] == [bytes(128)] * 16 and got_proofs[1] == [bytes(48)] * 16
        for i in (0, 2):
            assert cell_ints(got_cells[i]) == cells(fs[i], 5, 2)
            assert got_proofs[i] == [cell_proof(setup, to_coeffs(fs[i], 5), k, 5, 2) for k in range(16)]
    eng.set_cells_chunk(0)


def test_return_codes(eng, mono):
    lib, su = eng.lib, mono(2)
    blob, cells_out, pf, st = bytes(128), C.create_string_buffer(256), C.create_string_buffer(48 * 8), C.create_string_buffer(1)
    assert lib.nbls_kzg_compute_cells_and_proofs(eng.h, su.h, 0, 0, blob, cells_out, pf, st) == EINVAL
    assert lib.nbls_kzg_compute_cells_and_proofs(eng.h, su.h, 3, 1, blob, cells_out, pf, st) == EINVAL          # log2_cell > log2_n
    assert lib.nbls_kzg_compute_cells_and_proofs(eng.h, su.h, 0, 1, blob, cells_out, None, st) == EINVAL
    assert lib.nbls_kzg_compute_cells_and_proofs(eng.h, mono(12).h, 2, 1, blob, cells_out, pf, st) == EINVAL          # 2^11 rows of 2^12 scalars: above one pass
    assert lib.nbls_kzg_compute_cells_and_proofs(eng.h, su.h, 0, 1, blob, cells_out, pf, None) == 0          # status == NULL; the zero polynomial
    assert cells_out.raw == bytes(256) and pf.raw == ZERO48 * 8
    assert lib.nbls_kzg_compute_cells(eng.h, 2, 0, 0, None, None, None) == 0
    assert lib.nbls_kzg_compute_cells(eng.h, 2, 3, 1, blob, cells_out, st) == EINVAL
