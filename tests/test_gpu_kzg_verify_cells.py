"""nbls_kzg_verify_cells on the GPU (-m gpu).  Expected verdicts come from Python integers and kzg_cases.Setup's test-only tau, never from the call under test: cells from
kzg_cells_cases.cells, a cell's proof [q_k(tau)]G1 as one multiple of the generator from the oracle, [tau^c]G2 from the oracle.  Every proof costs an oracle multiplication,
so large calls repeat a pool of (cell, proof) pairs, which the interface allows.

Shapes (log2_n, log2_cell): (1,0) c = 1, no stage, M = 4; (2,1) two lanes per cell; (5,5) M = 2, two cells per wavefront; (8,3) eight cells per wavefront; (7,6) one cell per
wavefront; (6,0) for the comparison with nbls_kzg_verify_proofs; (12,6) the mainnet size, cells and proofs from the device's own prover."""
import ctypes as C
import importlib
import random
import pytest
from goldenio import hx
from kzg_cases import R, M256, NOT_VERIFIED, NON_CANONICAL, ZERO48, Setup, b32, blob_bytes
from kzg_cells_cases import cell_shift, monomial_setup
from kzg_verify_cells_cases import Blob, Call, random_blob, cells_per_blob, with_element, bumped

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
EDECODE = -5
SHAPES = [(1, 0), (2, 1), (5, 5), (8, 3), (7, 6)]


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


@pytest.fixture(scope='module')
def tau_c(setup):
    """log2_cell -> the compressed [tau^c]G2"""
    made = {}

    def get(log2_cell):
        if log2_cell not in made:
            made[log2_cell] = setup.tau_g2(pow(setup.tau, 1 << log2_cell, R))
        return made[log2_cell]
    return get


@pytest.fixture(scope='module')
def world(setup):
    """(log2_n, log2_cell) -> two random blobs of that shape with their commitments and cells (proofs on demand), made once and left unchanged"""
    made = {}

    def get(log2_n, log2_cell):
        if (log2_n, log2_cell) not in made:
            rnd = random.Random(8000 + 16 * log2_n + log2_cell)
            made[log2_n, log2_cell] = [random_blob(setup, log2_n, log2_cell, rnd) for _ in range(2)]
        return made[log2_n, log2_cell]
    return get


@pytest.fixture(scope='module')
def bad_points(golden):
    vec = golden['codec']['g1']
    return {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}


def verify(eng, mono, tau_c, shape, call, seed=SEED, per_item=True, tau=None):
    log2_n, log2_cell = shape
    cs, ci, ki, cells, proofs = call.args()
    return eng.kzg_verify_cells(mono(log2_n), log2_cell, cs, ci, ki, cells, proofs, tau_c(log2_cell) if tau is None else tau, seed, per_item)


def expect(eng, mono, tau_c, shape, call, want, tau=None):
    """the statuses with the per-cell pass, and the same verdict from the combined check alone"""
    ok, st = verify(eng, mono, tau_c, shape, call, tau=tau)
    assert list(st) == want
    assert ok == (not any(want))
    assert verify(eng, mono, tau_c, shape, call, per_item=False, tau=tau) == (ok, None)


def some_cells(blobs, shape, count, rnd):
    """a call of `count` cells drawn from both blobs (repeats where the blobs have fewer)"""
    m, call = cells_per_blob(*shape), Call(blobs)
    for j in range(count):
        call.add(j % 2, rnd.randrange(m))
    return call


@pytest.mark.parametrize('shape', SHAPES)
def test_every_cell_of_two_blobs(eng, mono, tau_c, world, shape):
    call = Call(world(*shape)).add_all(random.Random(8100))
    n = 2 * cells_per_blob(*shape)
    assert len(call.cells) == n
    expect(eng, mono, tau_c, shape, call, [0] * n)


@pytest.mark.parametrize('shape,count', [((8, 3), 1), ((8, 3), 37), ((8, 3), 129), ((7, 6), 1), ((7, 6), 5), ((2, 1), 3)])
def test_one_cell_alone_and_ragged_counts(eng, mono, tau_c, world, shape, count):
    """a workgroup takes 256 / c cells in the rows mode and four times as many in the sum mode: none of these counts is a multiple"""
    call = some_cells(world(*shape), shape, count, random.Random(8200 + count))
    expect(eng, mono, tau_c, shape, call, [0] * count)
    k = count // 2
    call.cells[k] = bumped(call.cells[k], 0)          # (the same cell elsewhere in the call keeps its bytes and stays valid)
    expect(eng, mono, tau_c, shape, call, [NOT_VERIFIED if j == k else 0 for j in range(count)])


def test_three_thousand_cells_from_a_pool(eng, mono, tau_c, world):
    """3001 cells at (8,3): the sum mode's lane groups walk four cells each and 24 partial rows are added.  Then one pooled cell is changed in one element wherever it occurs"""
    shape, rnd = (8, 3), random.Random(8300)
    blobs, m = world(*shape), cells_per_blob(8, 3)
    call = Call(blobs)
    for _ in range(3001):
        call.add(rnd.randrange(2), rnd.randrange(m))
    expect(eng, mono, tau_c, shape, call, [0] * 3001)
    b, k = call.ci[1500], call.ki[1500]
    hit = [j for j in range(3001) if (call.ci[j], call.ki[j]) == (b, k)]
    assert 1 < len(hit) < 100
    changed = bumped(blobs[b].cell(k), 5)
    for j in hit:
        call.cells[j] = changed
    expect(eng, mono, tau_c, shape, call, [NOT_VERIFIED if j in hit else 0 for j in range(3001)])


@pytest.mark.parametrize('shape', [(8, 3), (7, 6)])
@pytest.mark.parametrize('fault', ['element', 'proof of another cell', 'cell_index', 'commitment_index', 'two proofs exchanged'])
def test_each_way_to_be_wrong_between_good_neighbours(eng, mono, tau_c, world, shape, fault):
    blobs, m = world(*shape), cells_per_blob(*shape)
    call = Call(blobs)
    for b, k in [(0, 0), (1, 1), (0, 2), (1, m - 1), (0, 3), (1, 0), (0, m - 1)]:
        call.add(b, k)
    # At N = 2 c (the shape (7,6)) the floor quotient of p by X^c - s is the upper half of p's coefficients whatever s is: ALL cells of a blob have one and the same proof.
    # There "another cell" is a cell of the other blob, and an exchange inside one blob changes no byte (it is accepted; the exchange across the blobs is the fault)
    one_proof = blobs[0].proof(1) == blobs[0].proof(2)
    assert one_proof == (shape == (7, 6))
    wrong = {2}
    if fault == 'element':
        call.cells[2] = bumped(call.cells[2], (1 << shape[1]) - 1)
    elif fault == 'proof of another cell':
        call.proofs[2] = blobs[1].proof(1) if one_proof else blobs[0].proof(1)
    elif fault == 'cell_index':
        call.ki[2] = 1
    elif fault == 'commitment_index':
        call.ci[2] = 1
    else:          # cells 2 and 4 are of blob 0: the weights are per cell, so the exchange does not cancel in the sums
        call.proofs[2], call.proofs[4] = call.proofs[4], call.proofs[2]
        wrong = {2, 4}
        if one_proof:
            expect(eng, mono, tau_c, shape, call, [0] * 7)
            call.proofs[1], call.proofs[2] = call.proofs[2], call.proofs[1]
            wrong = {1, 2}
    expect(eng, mono, tau_c, shape, call, [NOT_VERIFIED if j in wrong else 0 for j in range(7)])


@pytest.mark.parametrize('shape', [(8, 3), (7, 6), (1, 0)])
def test_zero_points(eng, mono, tau_c, world, setup, shape):
    log2_n, log2_cell = shape
    m, rnd = cells_per_blob(*shape), random.Random(8400 + log2_n)
    zero = Blob(setup, [0] * (1 << log2_n), log2_n, log2_cell)
    assert zero.commitment == ZERO48 and zero.proof(0) == ZERO48 and zero.cell(m - 1) == bytes(32 << log2_cell)
    alone = Call([zero])
    for k in (0, m - 1, 1):
        alone.add(0, k)
    expect(eng, mono, tau_c, shape, alone, [0, 0, 0])          # A = B = the zero point
    mixed = Call([world(*shape)[0], zero])
    for b, k in [(0, 0), (1, 0), (0, m - 1), (1, m - 1)]:
        mixed.add(b, k)
    expect(eng, mono, tau_c, shape, mixed, [0] * 4)
    low = random_blob(setup, log2_n, log2_cell, rnd, degree=1 << log2_cell)          # degree < c: every quotient is zero, the commitment is not
    assert low.commitment != ZERO48 and low.proof(1) == ZERO48
    call = Call([low, world(*shape)[1]])
    for b, k in [(0, 0), (1, 1), (0, m - 1), (0, 1)]:
        call.add(b, k)
    expect(eng, mono, tau_c, shape, call, [0] * 4)
    only = Call([low]).add_all()          # every proof of the call is the zero point: A is, B must be
    expect(eng, mono, tau_c, shape, only, [0] * m)
    only.cells[1] = bumped(only.cells[1], 0)
    expect(eng, mono, tau_c, shape, only, [0, NOT_VERIFIED] + [0] * (m - 2))
    call.cells[2] = bumped(call.cells[2], 0)          # a zero proof holds exactly when the point on the right is the zero point
    expect(eng, mono, tau_c, shape, call, [0, 0, NOT_VERIFIED, 0])
    call = Call(world(*shape))
    for b, k in [(0, 0), (1, 1), (0, 1)]:
        call.add(b, k)
    call.proofs[1] = ZERO48          # an ordinary cell with the zero proof
    expect(eng, mono, tau_c, shape, call, [0, NOT_VERIFIED, 0])


@pytest.mark.parametrize('shape', [(8, 3), (7, 6)])
def test_refusals_between_good_cells(eng, mono, tau_c, world, bad_points, shape):
    blobs, m, c = world(*shape), cells_per_blob(*shape), 1 << shape[1]

    def base():
        call = Call(blobs)
        for b, k in [(0, 0), (1, 1), (0, 2), (1, m - 1), (0, 3), (1, 0)]:
            call.add(b, k)
        return call
    call = base()
    call.cells[1] = with_element(call.cells[1], c - 1, R)
    call.cells[4] = with_element(call.cells[4], 0, M256)
    expect(eng, mono, tau_c, shape, call, [0, NON_CANONICAL, 0, 0, NON_CANONICAL, 0])
    for name, code in (('subgroup', 3), ('noroot', 4)):
        call = base()
        call.commitments[1] = bad_points[name]          # every cell that names it, and no other
        expect(eng, mono, tau_c, shape, call, [0, code, 0, code, 0, code])
        call = base()
        call.proofs[2] = bad_points[name]
        expect(eng, mono, tau_c, shape, call, [0, 0, 10 + code, 0, 0, 0])
    call = base()          # the order of precedence: the commitment, then the proof, then the elements
    call.commitments[1] = bad_points['noroot']
    call.proofs[1] = bad_points['subgroup']
    call.cells[1] = with_element(call.cells[1], 0, R)
    call.proofs[2] = bad_points['noroot']
    call.cells[2] = with_element(call.cells[2], 1, M256)
    expect(eng, mono, tau_c, shape, call, [0, 4, 14, 4, 0, 4])
    call = base()          # a commitment that no cell names is decoded and otherwise ignored
    call.commitments.append(bad_points['subgroup'])
    expect(eng, mono, tau_c, shape, call, [0] * 6)


def test_tau_c_g2_rules(eng, pkg, mono, tau_c, world, setup):
    shape = (8, 3)
    call = some_cells(world(*shape), shape, 5, random.Random(8500))
    cs, ci, ki, cells, proofs = call.args()
    arr = lambda v: (C.c_uint32 * len(v))(*v)
    for tau in (b'\xc0' + bytes(95), b'\x00' * 96, bytes([0x9f]) + b'\xff' * 95):          # the zero point; not a compressed point; x >= p
        ok, st = C.c_int(77), C.create_string_buffer(b'\x55' * 5, 5)
        r = eng.lib.nbls_kzg_verify_cells(eng.h, mono(8).h, 3, 2, b''.join(cs), 5, arr(ci), arr(ki), b''.join(cells), b''.join(proofs), tau, SEED, C.byref(ok), st)
        assert r == EDECODE and ok.value == 77 and st.raw == b'\x55' * 5
        with pytest.raises(pkg.NblsError):
            verify(eng, mono, tau_c, shape, call, tau=tau)
    expect(eng, mono, tau_c, shape, call, [NOT_VERIFIED] * 5, tau=setup.tau_g2())          # [tau]G2 where [tau^8]G2 belongs
    expect(eng, mono, tau_c, shape, call, [0] * 5)


def test_one_element_cells_against_the_opening_verifier(eng, mono, tau_c, world, setup):
    """at c = 1 a cell proof is the opening at z = h_k with y the cell's element, and tau^c = tau: the same tuples go through nbls_kzg_verify_proofs"""
    shape = (6, 0)
    blobs, m, rnd = world(*shape), cells_per_blob(6, 0), random.Random(8600)
    call = Call(blobs)
    for j in range(9):
        call.add(j % 2, rnd.randrange(m))
    cs, ci, ki, cells, proofs = call.args()
    zs = [cell_shift(k, 6, 0) for k in ki]
    assert tau_c(0) == setup.tau_g2()
    for tamper in (False, True):
        if tamper:
            cells[4] = bumped(cells[4], 0)
        want = [NOT_VERIFIED if tamper and j == 4 else 0 for j in range(9)]
        ok, st = eng.kzg_verify_cells(mono(6), 0, cs, ci, ki, cells, proofs, tau_c(0), SEED)
        ok2, st2 = eng.kzg_verify_proofs([cs[i] for i in ci], zs, [int.from_bytes(v, 'big') for v in cells], proofs, setup.tau_g2(), SEED)
        assert list(st) == want and list(st2) == want and ok == ok2 == (not tamper)


@pytest.mark.parametrize('shape', [(8, 3), (12, 6)])
def test_against_the_prover(eng, mono, tau_c, setup, shape):
    """a cross-check, not an oracle: cells and proofs come from nbls_kzg_compute_cells_and_proofs; the commitment from Python"""
    log2_n, log2_cell = shape
    rnd = random.Random(8700 + log2_n)
    f = [rnd.randrange(R) for _ in range(1 << log2_n)]
    (cells,), (proofs,), st = eng.kzg_compute_cells_and_proofs(mono(log2_n), log2_cell, [blob_bytes(f)])
    m = cells_per_blob(*shape)
    assert list(st) == [0] and len(cells) == m == len(proofs)
    order = list(range(m))
    rnd.shuffle(order)
    args = [[setup.commit(f, log2_n)], [0] * m, order, [cells[k] for k in order], [proofs[k] for k in order], tau_c(log2_cell), SEED]
    assert eng.kzg_verify_cells(mono(log2_n), log2_cell, *args) == (True, bytes(m))
    assert eng.kzg_verify_cells(mono(log2_n), log2_cell, *args, per_item=False) == (True, None)
    j = m // 3
    flipped = bytearray(args[3][j])
    flipped[31] ^= 1          # the lowest byte of element 0
    args[3][j] = bytes(flipped)
    assert eng.kzg_verify_cells(mono(log2_n), log2_cell, *args) == (False, bytes(NOT_VERIFIED if i == j else 0 for i in range(m)))
    assert eng.kzg_verify_cells(mono(log2_n), log2_cell, *args, per_item=False) == (False, None)


def test_the_seed(eng, mono, tau_c, world):
    shape = (7, 6)
    call = some_cells(world(*shape), shape, 6, random.Random(8800))
    bad = some_cells(world(*shape), shape, 6, random.Random(8800))
    bad.cells[3] = bumped(bad.cells[3], 17)
    want = [0, 0, 0, NOT_VERIFIED, 0, 0]
    for seed in (SEED, bytes(32), b'\xff' * 32):
        assert verify(eng, mono, tau_c, shape, call, seed=seed) == verify(eng, mono, tau_c, shape, call, seed=seed) == (True, bytes(6))
        assert verify(eng, mono, tau_c, shape, bad, seed=seed) == verify(eng, mono, tau_c, shape, bad, seed=seed) == (False, bytes(want))
    for _ in range(3):          # a seed from the OS on every call
        assert verify(eng, mono, tau_c, shape, call, seed=None) == (True, bytes(6))
        assert verify(eng, mono, tau_c, shape, bad, seed=None) == (False, bytes(want))
        assert verify(eng, mono, tau_c, shape, bad, seed=None, per_item=False) == (False, None)


def test_both_verifiers_and_the_shared_tables_on_one_context(pkg, mono, tau_c, world, setup):
    """the two verifiers alternate on a context of its own, each through its per-item pass (the shared tail on SB_KZG_* and on SB_KZGV_*), between calls that use the tables the
    other made: the inverse roots of size 8 are made by nbls_kzg_verify_cells at (8,3) and read by nbls_fr_ntt(3), or the other way round on a second context"""
    from kzg_cells_cases import to_coeffs
    ints = lambda row: [int.from_bytes(v, 'big') for v in row]
    c83 = some_cells(world(8, 3), (8, 3), 37, random.Random(8200 + 37))
    c83.cells[18] = bumped(c83.cells[18], 0)
    c21 = some_cells(world(2, 1), (2, 1), 3, random.Random(8200 + 3))
    nine, rnd = Call(world(6, 0)), random.Random(8600)          # cells of one element are openings: the tuples of test_one_element_cells_against_the_opening_verifier
    for j in range(9):
        nine.add(j % 2, rnd.randrange(cells_per_blob(6, 0)))
    cs, ci, ki, cells, proofs = nine.args()
    tuples = [[cs[i] for i in ci], [cell_shift(k, 6, 0) for k in ki], [int.from_bytes(v, 'big') for v in cells], proofs]
    tuples[2][4] = (tuples[2][4] + 1) % R
    polys = [[rnd.randrange(R) for _ in range(8)] for _ in range(2)]
    blob = world(8, 3)[0]

    def calls(eng):
        def ntt():
            coef, st = eng.fr_ntt(3, polys, False)
            back, st2 = eng.fr_ntt(3, [ints(v) for v in coef], True)
            return [ints(v) for v in coef], st, [ints(v) for v in back], st2
        return {1: lambda: verify(eng, mono, tau_c, (8, 3), c83),
                2: ntt,
                3: lambda: eng.kzg_verify_proofs(*tuples, setup.tau_g2(), SEED),
                4: lambda: verify(eng, mono, tau_c, (2, 1), c21),
                5: lambda: eng.kzg_compute_cells_and_proofs(mono(8), 3, [blob_bytes(blob.f)]),
                6: lambda: eng.kzg_verify_proofs(*[v[:2] for v in tuples], setup.tau_g2(), SEED),
                7: lambda: verify(eng, mono, tau_c, (8, 3), c83)}
    st83 = bytes(NOT_VERIFIED if j == 18 else 0 for j in range(37))
    want = {1: (False, st83),
            2: ([to_coeffs(f, 3) for f in polys], [0, 0], polys, [0, 0]),
            3: (False, bytes(NOT_VERIFIED if j == 4 else 0 for j in range(9))),
            4: (True, bytes(3)),
            5: ([[blob.cell(k) for k in range(64)]], [[blob.proof(k) for k in range(64)]], bytes(1)),
            6: (True, bytes(2)),
            7: (False, st83)}
    runs = []
    for order in ([1, 2, 3, 4, 5, 6, 7], [2, 1, 3, 4, 5, 6, 7]):
        eng = pkg.Engine(0)          # every table and every slot of this context is made here
        got = {}
        for k in order:
            got[k] = calls(eng)[k]()
            assert got[k] == want[k], (order, k)
        eng.close()
        runs.append(got)
    assert runs[0] == runs[1]
