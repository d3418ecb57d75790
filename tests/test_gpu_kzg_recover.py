"""PeerDAS recovery on the GPU (-m gpu): nbls_kzg_recover_cells and nbls_kzg_recover_cells_and_proofs against Python integers (kzg_cells_cases.py: the cells of the original
blob; kzg_recover_cases.py: the specification's route, for inputs that are no blob's cells), kzg_cases.py's test-only trusted setup (with tau known a cell's proof is one
multiple of the generator from the oracle) and the bytes of the existing calls for the original blob.  Every comparison is exact.

The recovery kernel has kzg_ntt_kernel's 512 lanes per blob: up to N = 512 a lane owns at most one element, at 1024 two, at 2048 four, at 4096 eight -- hence (9,6), (10,4),
(11,6) and (12,6); (6,0) has 128 one-element cells, (5,5) two cells, of which one alone is exactly half."""
import ctypes as C
import importlib
import random
import pytest
from kzg_cases import R, M256, NON_CANONICAL, ZERO48, Setup, blob_bytes
from kzg_cells_cases import to_evals, cells, cell_proof, monomial_setup, rows
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, n_cells, recover, patterns

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
    """log2_n -> the device-resident monomial basis of that size, created on first use"""
    made = {}

    def get(log2_n):
        if log2_n not in made:
            made[log2_n] = eng.kzg_monomial_setup(log2_n, monomial_setup(setup, log2_n))
        return made[log2_n]
    yield get
    for s in made.values():
        s.close()


def cell_bytes(cell_lists):
    return [rows(c) for c in cell_lists]


def blob_of(rnd, log2_n, log2_cell):
    """a random polynomial -> (coefficients, its cells as integers, its cells as bytes, the blob's bytes)"""
    coef = [rnd.randrange(R) for _ in range(1 << log2_n)]
    f = to_evals(coef, log2_n)
    cs = cells(f, log2_n, log2_cell)
    return coef, cs, cell_bytes(cs), blob_bytes(f)


def pick(cb, idx):
    return [cb[k] for k in idx]


# ---- (a) the cells

@pytest.mark.parametrize('log2_n,log2_cell', [(1, 0), (2, 1), (6, 0), (5, 5), (8, 3), (9, 6), (10, 4), (11, 6)])
def test_recover_cells_every_pattern(eng, log2_n, log2_cell):
    rnd = random.Random(900 + 16 * log2_n + log2_cell)
    coef, cs, cb, blob = blob_of(rnd, log2_n, log2_cell)
    pats = patterns(log2_n, log2_cell, rnd)
    if log2_n == 5:
        pats += [('cell 0 alone', [0]), ('cell 1 alone', [1])]
    got, st = eng.kzg_recover_cells(log2_n, log2_cell, [idx for _, idx in pats], [pick(cb, idx) for _, idx in pats])
    assert st == bytes(len(pats))
    for (name, _), g in zip(pats, got):
        assert g == cb, name
    assert (got[:1], bytes(1)) == eng.kzg_compute_cells(log2_n, log2_cell, [blob])
    alone, st = eng.kzg_recover_cells(log2_n, log2_cell, [pats[-1][1]], [pick(cb, pats[-1][1])])
    assert (alone, st) == ([cb], bytes(1))


def test_recover_cells_mainnet_size_once(eng):
    rnd = random.Random(990)
    coef, cs, cb, blob = blob_of(rnd, 12, 6)
    idx = rnd.sample(range(128), 64)
    got, st = eng.kzg_recover_cells(12, 6, [idx], [pick(cb, idx)])
    assert st == bytes(1) and got == [cb]


# ---- (b) cells and proofs

@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (6, 0), (5, 5), (8, 3)])
def test_recover_cells_and_proofs(eng, setup, mono, log2_n, log2_cell):
    rnd = random.Random(1000 + 16 * log2_n + log2_cell)
    m = n_cells(log2_n, log2_cell)
    coef, cs, cb, blob = blob_of(rnd, log2_n, log2_cell)
    pats = patterns(log2_n, log2_cell, rnd)
    if log2_n == 5:
        pats += [('cell 0 alone', [0]), ('cell 1 alone', [1])]
    want_proofs = [cell_proof(setup, coef, k, log2_n, log2_cell) for k in range(m)]
    got_cells, got_proofs, st = eng.kzg_recover_cells_and_proofs(mono(log2_n), log2_cell, [idx for _, idx in pats], [pick(cb, idx) for _, idx in pats])
    assert st == bytes(len(pats))
    for (name, _), gc, gp in zip(pats, got_cells, got_proofs):
        assert gc == cb and gp == want_proofs, name
    assert (got_cells[:1], got_proofs[:1], bytes(1)) == eng.kzg_compute_cells_and_proofs(mono(log2_n), log2_cell, [blob])


def test_mainnet_blob_from_64_shuffled_cells(eng, mono):
    """equal to the bytes of kzg_compute_cells_and_proofs for that blob, which has its oracle test (test_gpu_kzg_cells.py): the 128 oracle multiplications are not repeated"""
    rnd = random.Random(1100)
    coef, cs, cb, blob = blob_of(rnd, 12, 6)
    idx = rnd.sample(range(128), 64)
    got = eng.kzg_recover_cells_and_proofs(mono(12), 6, [idx], [pick(cb, idx)])
    assert got == eng.kzg_compute_cells_and_proofs(mono(12), 6, [blob]) and got[2] == bytes(1) and got[0] == [cb]


def test_three_blobs_with_different_counts_and_a_refused_one_between(eng, mono):
    rnd = random.Random(1110)
    L, lc, m = 6, 2, 32
    blobs = [blob_of(rnd, L, lc) for _ in range(3)]
    idxs = [rnd.sample(range(m), m // 2), rnd.sample(range(m), m // 2 + 1), rnd.sample(range(m), m)]
    given = [pick(b[2], idx) for b, idx in zip(blobs, idxs)]
    short = rnd.sample(range(m), m // 2 - 1)
    got = eng.kzg_recover_cells_and_proofs(mono(L), lc, [idxs[0], idxs[1], short, idxs[2]], [given[0], given[1], pick(blobs[0][2], short), given[2]])
    assert got[2] == bytes([0, 0, BAD_CELLS, 0])
    assert got[0][2] == [bytes(32 << lc)] * m and got[1][2] == [bytes(48)] * m
    for j, i in ((0, 0), (1, 1), (3, 2)):
        alone = eng.kzg_recover_cells_and_proofs(mono(L), lc, [idxs[i]], [given[i]])
        assert alone == ([got[0][j]], [got[1][j]], bytes(1)) and alone[0] == [blobs[i][2]]


# ---- (c) the statuses, each between two good blobs

@pytest.mark.parametrize('log2_n,log2_cell', [(2, 1), (5, 5), (8, 3), (10, 4)])
def test_statuses(eng, mono, log2_n, log2_cell):
    rnd = random.Random(1200 + 16 * log2_n + log2_cell)
    m, n, c = n_cells(log2_n, log2_cell), 1 << log2_n, 1 << log2_cell
    coef, cs, cb, blob = blob_of(rnd, log2_n, log2_cell)
    half = rnd.sample(range(m), m // 2)
    more = half + [next(k for k in range(m) if k not in half)]
    take = lambda idx: [list(cs[k % m]) for k in idx]

    def changed(idx, e, j, v):
        g = take(idx)
        g[e][j] = v if v is not None else (g[e][j] + 1) % R
        return idx, g
    cases = [('short', (half[:-1], take(half[:-1])), BAD_CELLS), ('twice', (half[1:] + [half[-1]] * 2, take(half[1:] + [half[-1]] * 2)), BAD_CELLS),
             ('index = M', (half[:-1] + [m], take(half[:-1] + [m])), BAD_CELLS), ('none', ([], []), BAD_CELLS),
             ('element = r', changed(half, len(half) - 1, c - 1, R), NON_CANONICAL), ('element = 2^256 - 1', changed(more, len(more) - 1, 0, M256), NON_CANONICAL),
             ('short and non-canonical', (half[:-1], [[R] * c for _ in half[:-1]]), BAD_CELLS), ('changed, half + 1', changed(more, 0, 0, None), INCONSISTENT)]
    idx, g = changed(more, 0, 0, None)
    g[1][0] = R
    cases.append(('non-canonical and inconsistent', (idx, g), NON_CANONICAL))
    flip = changed(half, 0, 0, None)
    st_ref, flip_cells, _ = recover(flip[0], flip[1], log2_n, log2_cell)
    assert st_ref == 0
    proofs = log2_n <= 8
    zero_cells, zero_proofs = [bytes(32 * c)] * m, [bytes(48)] * m
    for name, (bidx, bgiven), code in cases:
        args = ([half, bidx, flip[0]], [pick(cb, half), cell_bytes(bgiven), cell_bytes(flip[1])])
        if proofs:
            got, pf, st = eng.kzg_recover_cells_and_proofs(mono(log2_n), log2_cell, *args)
            assert pf[1] == zero_proofs and len(pf[0]) == m and bytes(48) not in pf[0] + pf[2], name
        else:
            got, st = eng.kzg_recover_cells(log2_n, log2_cell, *args)
        assert st == bytes([0, code, 0]), name
        assert got == [cb, zero_cells, cell_bytes(flip_cells)], name          # exactly half with one changed element: status 0 and the reference's recovery of the changed data


def test_zero_polynomial_and_degree_below_c_from_half_the_cells(eng, mono):
    rnd = random.Random(1300)
    L, lc, m = 6, 3, 16
    coefs = [[0] * 64, [rnd.randrange(1, R) for _ in range(8)] + [0] * 56]
    cbs = [cell_bytes(cells(to_evals(co, L), L, lc)) for co in coefs]
    idxs = [rnd.sample(range(m), m // 2) for _ in coefs]
    got_cells, got_proofs, st = eng.kzg_recover_cells_and_proofs(mono(L), lc, idxs, [pick(cb, idx) for cb, idx in zip(cbs, idxs)])
    assert st == bytes(2) and got_cells == cbs and got_proofs == [[ZERO48] * m] * 2
    assert got_cells[0] == [bytes(256)] * m


def test_chunks_give_the_same_bytes(pkg, mono):
    rnd = random.Random(1400)
    L, lc, m = 5, 2, 16
    blobs = [blob_of(rnd, L, lc) for _ in range(3)]
    idxs = [rnd.sample(range(m), m // 2 + i) for i in range(3)]
    other = pkg.Engine(0)
    runs = []
    for chunk in (1, 2, 0):
        other.set_cells_chunk(chunk)
        runs.append(other.kzg_recover_cells_and_proofs(mono(L), lc, idxs, [pick(b[2], idx) for b, idx in zip(blobs, idxs)]))
    want = other.kzg_compute_cells_and_proofs(mono(L), lc, [b[3] for b in blobs])
    other.close()
    assert runs[0] == runs[1] == runs[2] == want and want[2] == bytes(3)


def test_against_the_existing_verifier(eng, setup, mono):
    rnd = random.Random(1500)
    L, lc, m = 8, 3, 64
    coef, cs, cb, blob = blob_of(rnd, L, lc)
    idx = rnd.sample(range(m), m // 2)
    got_cells, got_proofs, st = eng.kzg_recover_cells_and_proofs(mono(L), lc, [idx], [pick(cb, idx)])
    assert st == bytes(1)
    commitment = setup.commit(to_evals(coef, L), L)
    ok, vst = eng.kzg_verify_cells(mono(L), lc, [commitment], [0] * m, list(range(m)), got_cells[0], got_proofs[0], setup.tau_g2(pow(setup.tau, 1 << lc, R)), seed=SEED)
    assert ok and vst == bytes(m)


# ---- (d) return codes

def test_return_codes(eng, mono):
    lib, su = eng.lib, mono(2)
    u32 = C.c_uint32
    off, idx, x = (u32 * 2)(0, 4), (u32 * 4)(0, 1, 2, 3), bytes(256)
    out, pf, st = C.create_string_buffer(256), C.create_string_buffer(48 * 8), C.create_string_buffer(2)
    f, g = lib.nbls_kzg_recover_cells, lib.nbls_kzg_recover_cells_and_proofs
    assert f(eng.h, 2, 0, 1, off, idx, x, out, None) == 0 and out.raw == bytes(256)          # status == NULL; the zero polynomial from half of its cells
    assert g(eng.h, su.h, 0, 1, off, idx, x, out, pf, None) == 0 and out.raw == bytes(256) and pf.raw == ZERO48 * 8
    assert f(eng.h, 2, 0, 0, None, None, None, None, None) == 0          # n = 0: the cells form answers NBLS_OK
    assert g(eng.h, su.h, 0, 0, off, idx, x, out, pf, st) == EINVAL          # ... the proofs form does not
    for bad in ([None, 2, 0, 1, off, idx, x, out, st], [eng.h, 2, 0, 1, None, idx, x, out, st], [eng.h, 2, 0, 1, off, None, x, out, st], [eng.h, 2, 0, 1, off, idx, None, out, st],
                [eng.h, 2, 0, 1, off, idx, x, None, st], [eng.h, 0, 0, 1, off, idx, x, out, st], [eng.h, 13, 6, 1, off, idx, x, out, st], [eng.h, 2, 3, 1, off, idx, x, out, st],
                [eng.h, 12, 0, 1, off, idx, x, out, st],          # 2^13 cells: more than the table of roots holds
                [eng.h, 2, 0, 1, (u32 * 2)(1, 4), idx, x, out, st], [eng.h, 2, 0, 2, (u32 * 3)(0, 4, 3), idx, x, out, st],
                [eng.h, 12, 6, 4097, off, idx, x, out, st]):          # more than 2^24 elements of blobs
        assert f(*bad) == EINVAL, bad[1:4]
    for bad in ([None, su.h, 0, 1, off, idx, x, out, pf, st], [eng.h, None, 0, 1, off, idx, x, out, pf, st], [eng.h, su.h, 0, 1, None, idx, x, out, pf, st],
                [eng.h, su.h, 0, 1, off, None, x, out, pf, st], [eng.h, su.h, 0, 1, off, idx, None, out, pf, st], [eng.h, su.h, 0, 1, off, idx, x, None, pf, st],
                [eng.h, su.h, 0, 1, off, idx, x, out, None, st], [eng.h, su.h, 3, 1, off, idx, x, out, pf, st], [eng.h, su.h, 0, 1, (u32 * 2)(1, 4), idx, x, out, pf, st],
                [eng.h, su.h, 0, 2, (u32 * 3)(0, 4, 3), idx, x, out, pf, st],
                [eng.h, mono(12).h, 2, 1, off, idx, x, out, pf, st]):          # 2^11 rows of 2^12 scalars: above one pass of the batched MSM
        assert g(*bad) == EINVAL, bad[2:4]
    # no cell given at all: index and cell pointers may be NULL, and every blob is refused
    assert f(eng.h, 2, 0, 2, (u32 * 3)(0, 0, 0), None, None, out, st) == 0 and st.raw == bytes([BAD_CELLS] * 2)
    assert g(eng.h, su.h, 0, 1, (u32 * 2)(0, 0), None, None, out, pf, st) == 0 and st.raw[0] == BAD_CELLS and pf.raw == bytes(48 * 8)
