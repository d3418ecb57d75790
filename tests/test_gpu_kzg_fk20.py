"""FK20 on the GPU (-m gpu): nbls_kzg_fk20_create, nbls_kzg_compute_cells_and_proofs_fk20 and nbls_kzg_recover_cells_and_proofs_fk20 against the oracle (with tau known a
cell's proof is [q_k(tau)]G1: kzg_cells_cases.cell_proof) and against the existing calls, which have their own oracle tests: byte for byte the same cells, proofs and
statuses.  No expected value comes from the calls under test.

The shapes: (2,1) M = 4, n' = 2 (one term per fixed point); (5,5) n' = 1 (no pass at all); (6,0) c = 1, M = 128 (groups of one term in pass A, the scalars kernel with four
stripes a workgroup); (8,3) M = 64; (5,2) M = 16 for chunks and refusals; (12,6) the mainnet size."""
import ctypes as C
import importlib
import random
import pytest
from kzg_cases import R, M256, NON_CANONICAL, ZERO48, Setup, b32, blob_bytes
from kzg_cells_cases import to_evals, to_coeffs, cells, cell_proof, monomial_setup, rows
from kzg_recover_cases import BAD_CELLS, INCONSISTENT
from test_gpu_kzg_cells import proof_blobs, cell_ints

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
EINVAL = -1


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
    made = {}

    def get(log2_n):
        if log2_n not in made:
            made[log2_n] = eng.kzg_monomial_setup(log2_n, monomial_setup(setup, log2_n))
        return made[log2_n]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope='module')
def fk(eng, mono):
    """(log2_n, log2_cell) -> the FK20 handle of that shape, created on first use"""
    made = {}

    def get(log2_n, log2_cell):
        if (log2_n, log2_cell) not in made:
            made[(log2_n, log2_cell)] = eng.kzg_fk20_setup(mono(log2_n), log2_cell)
        return made[(log2_n, log2_cell)]
    yield get
    for s in made.values():
        s.close()


def blob_of(rnd, log2_n, log2_cell):
    """a random polynomial -> (coefficients, its values, its cells as bytes, the blob's bytes)"""
    coef = [rnd.randrange(R) for _ in range(1 << log2_n)]
    f = to_evals(coef, log2_n)
    return coef, f, [rows(c) for c in cells(f, log2_n, log2_cell)], blob_bytes(f)


@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (5, 5), (6, 0), (8, 3)])
def test_small_shapes(eng, setup, mono, fk, log2_n, log2_cell):
    rnd = random.Random(800 + 16 * log2_n + log2_cell)          # (the blobs of test_gpu_kzg_cells.py's test of the other form)
    cases = proof_blobs(log2_n, log2_cell, rnd)
    per = 2 << (log2_n - log2_cell)
    blobs = [blob_bytes(f) for f, _ in cases.values()]
    h = fk(log2_n, log2_cell)
    assert (h.log2_n, h.log2_cell) == (log2_n, log2_cell)
    got = eng.kzg_compute_cells_and_proofs_fk20(h, blobs)
    assert got[2] == bytes(len(cases))
    for (name, (f, coef)), cs, ps in zip(cases.items(), got[0], got[1]):
        assert cell_ints(cs) == cells(f, log2_n, log2_cell), name
        assert ps == [cell_proof(setup, coef, k, log2_n, log2_cell) for k in range(per)], name
        if name in ('zero', 'degree<c'):
            assert ps == [ZERO48] * per, name          # identities into pass B; non-zero sums of pass A that the matrix sends to the exact zero point
    assert got == eng.kzg_compute_cells_and_proofs(mono(log2_n), log2_cell, blobs)
    alone = eng.kzg_compute_cells_and_proofs_fk20(h, blobs[:1])
    assert alone == (got[0][:1], got[1][:1], bytes(1))


def test_mainnet_size(eng, setup, mono, fk):
    rnd = random.Random(2880)
    f = [rnd.randrange(R) for _ in range(4096)]
    coef = to_coeffs(f, 12)
    got = eng.kzg_compute_cells_and_proofs_fk20(fk(12, 6), [blob_bytes(f)])
    assert got == eng.kzg_compute_cells_and_proofs(mono(12), 6, [blob_bytes(f)]) and got[2] == bytes(1)
    for k in (0, 1, 64, 127):
        assert got[1][0][k] == cell_proof(setup, coef, k, 12, 6), k


def test_chunks_give_the_same_bytes(pkg, setup, mono, fk):
    rnd = random.Random(2895)
    blobs = [blob_bytes([rnd.randrange(R) for _ in range(32)]) for _ in range(3)]
    other = pkg.Engine(0)          # a fresh engine: its slots grow with the first chunk size it meets
    runs = []
    for chunk in (1, 2, 0):
        other.set_cells_chunk(chunk)
        runs.append(other.kzg_compute_cells_and_proofs_fk20(fk(5, 2), blobs))
    other.close()
    assert runs[0] == runs[1] == runs[2] and runs[0][2] == bytes(3)
    coef = to_coeffs([int.from_bytes(blobs[2][32 * j:32 * j + 32], 'big') for j in range(32)], 5)
    assert runs[0][1][2] == [cell_proof(setup, coef, k, 5, 2) for k in range(16)]


@pytest.mark.parametrize('where', [31, 13])
def test_a_refused_blob_between_two_good_ones(eng, setup, fk, where):
    """a non-canonical element in the last position, and one in the middle"""
    rnd = random.Random(2897 + where)
    fs = [[rnd.randrange(R) for _ in range(32)] for _ in range(3)]
    blobs = [blob_bytes(f) for f in fs]
    raw = bytearray(blobs[1]); raw[32 * where:32 * where + 32] = b32(M256 if where == 31 else R); blobs[1] = bytes(raw)
    want = [[cell_proof(setup, to_coeffs(fs[i], 5), k, 5, 2) for k in range(16)] for i in (0, 2)]
    try:
        for chunk in (0, 1):
            eng.set_cells_chunk(chunk)
            got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs_fk20(fk(5, 2), blobs)
            assert st == bytes([0, NON_CANONICAL, 0])
            assert got_cells[1] == [bytes(128)] * 16 and got_proofs[1] == [bytes(48)] * 16
            for i, w in zip((0, 2), want):
                assert cell_ints(got_cells[i]) == cells(fs[i], 5, 2) and got_proofs[i] == w
    finally:
        eng.set_cells_chunk(0)


@pytest.mark.parametrize('log2_n,log2_cell', [(5, 2), (8, 3)])
def test_recovery(eng, setup, mono, fk, log2_n, log2_cell):
    """from a random half and from half + 1 in shuffled order; a blob with too few cells and a contradicted one stand between good ones"""
    rnd = random.Random(3000 + 16 * log2_n + log2_cell)
    m = 2 << (log2_n - log2_cell)
    a, b = blob_of(rnd, log2_n, log2_cell), blob_of(rnd, log2_n, log2_cell)
    half, more, short = rnd.sample(range(m), m // 2), rnd.sample(range(m), m // 2 + 1), rnd.sample(range(m), m // 2 - 1)
    pick = lambda cb, idx: [cb[k] for k in idx]
    wrong = pick(b[2], more)
    first = bytearray(wrong[0]); first[31] ^= 1; wrong[0] = bytes(first)          # half + 1 cells, one element changed: no polynomial of degree < N has them all
    idxs = [half, short, more, more, half]
    given = [pick(a[2], half), pick(a[2], short), pick(b[2], more), wrong, pick(b[2], half)]
    got = eng.kzg_recover_cells_and_proofs_fk20(fk(log2_n, log2_cell), idxs, given)
    assert got[2] == bytes([0, BAD_CELLS, 0, INCONSISTENT, 0])
    assert got == eng.kzg_recover_cells_and_proofs(mono(log2_n), log2_cell, idxs, given)
    for i in (1, 3):
        assert got[0][i] == [bytes(32 << log2_cell)] * m and got[1][i] == [bytes(48)] * m
    for i, blob in ((0, a), (2, b), (4, b)):
        assert got[0][i] == blob[2] and got[1][i] == [cell_proof(setup, blob[0], k, log2_n, log2_cell) for k in range(m)], i


def test_handle_sharing_and_independence_from_neighbours(pkg, eng, setup, mono, fk):
    """one handle used by two engines; a verify_multiple call and a call of the other form give what they gave before and after FK20 calls of growing size"""
    from test_gpu_verify_multiple import random_sets
    rnd = random.Random(3100)
    sets = random_sets(eng, 5, rnd)
    blobs5 = [blob_bytes([rnd.randrange(R) for _ in range(32)]) for _ in range(2)]
    before = (eng.verify_multiple(sets[0], sets[1], sets[2], seed=SEED), eng.kzg_compute_cells_and_proofs(mono(5), 2, blobs5))
    assert before[0] == (True, bytes(5)) and before[1][2] == bytes(2)
    other = pkg.Engine(0)
    for n, (L, lc) in ((1, (5, 2)), (3, (5, 2)), (2, (8, 3)), (7, (5, 2))):
        blobs = [blob_bytes([rnd.randrange(R) for _ in range(1 << L)]) for _ in range(n)]
        mine = eng.kzg_compute_cells_and_proofs_fk20(fk(L, lc), blobs)
        assert mine == other.kzg_compute_cells_and_proofs_fk20(fk(L, lc), blobs) == eng.kzg_compute_cells_and_proofs(mono(L), lc, blobs)
        assert (eng.verify_multiple(sets[0], sets[1], sets[2], seed=SEED), eng.kzg_compute_cells_and_proofs(mono(5), 2, blobs5)) == before
    other.close()


def test_the_verifier_accepts_every_proof_and_rejects_an_exchanged_one(eng, setup, mono, fk):
    rnd = random.Random(3200)
    L, lc, m = 8, 3, 64
    a, b = blob_of(rnd, L, lc), blob_of(rnd, L, lc)
    got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs_fk20(fk(L, lc), [a[3], b[3]])
    assert st == bytes(2)
    commitment = setup.commit(a[1], L)
    tau_c = setup.tau_g2(pow(setup.tau, 1 << lc, R))
    ok, vst = eng.kzg_verify_cells(mono(L), lc, [commitment], [0] * m, list(range(m)), got_cells[0], got_proofs[0], tau_c, seed=SEED)
    assert ok and vst == bytes(m)
    proofs = list(got_proofs[0])
    proofs[17] = got_proofs[1][17]          # the proof of the same cell of a second blob
    ok, vst = eng.kzg_verify_cells(mono(L), lc, [commitment], [0] * m, list(range(m)), got_cells[0], proofs, tau_c, seed=SEED)
    assert not ok and vst == bytes([9 if k == 17 else 0 for k in range(m)])


def test_return_codes(eng, mono, fk):
    lib, h = eng.lib, fk(2, 1)
    blob, cells_out, pf, st, out = bytes(128), C.create_string_buffer(256), C.create_string_buffer(48 * 4), C.create_string_buffer(1), C.c_void_p(7)
    f, g = lib.nbls_kzg_compute_cells_and_proofs_fk20, lib.nbls_kzg_recover_cells_and_proofs_fk20
    assert f(eng.h, h.h, 0, blob, cells_out, pf, st) == EINVAL and f(eng.h, h.h, 1, blob, cells_out, None, st) == EINVAL and f(eng.h, None, 1, blob, cells_out, pf, st) == EINVAL
    assert f(eng.h, h.h, 1, blob, cells_out, pf, None) == 0          # status == NULL; the zero polynomial
    assert cells_out.raw == bytes(256) and pf.raw == ZERO48 * 4
    u32 = C.c_uint32
    assert g(eng.h, h.h, 0, (u32 * 1)(0), None, None, cells_out, pf, st) == EINVAL
    assert g(eng.h, h.h, 1, (u32 * 2)(0, 0), None, None, cells_out, pf, st) == 0 and st.raw[0] == BAD_CELLS and pf.raw == bytes(48 * 4)
    assert g(eng.h, h.h, 1, (u32 * 2)(0, 2), (u32 * 2)(0, 1), bytes(128), cells_out, pf, None) == 0 and pf.raw == ZERO48 * 4
    assert lib.nbls_kzg_fk20_create(eng.h, mono(2).h, 3, C.byref(out)) == EINVAL and out.value is None
    assert lib.nbls_kzg_fk20_create(eng.h, mono(12).h, 2, C.byref(out)) == EINVAL and out.value is None          # 2^11 cells of 2^12 elements: above one pass
    assert lib.nbls_set_tuning(eng.h, 21, 0) == EINVAL
