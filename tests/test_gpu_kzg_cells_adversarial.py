"""The three PeerDAS calls at the inputs their first tests left out (-m gpu): nbls_kzg_verify_cells, nbls_kzg_compute_cells[_and_proofs], nbls_kzg_recover_cells[_and_proofs].
The test-only tau is known (kzg_cases.py), so a cell tuple is the integers cm, q, I = I_k(tau) behind C = [cm]G1 and pi = [q]G1; it holds exactly when
q tau^c = cm - I + s_k q, and with a fixed seed the weights r_j are known too (kzg_cells_adversarial_cases.Forge restates the combined check in those integers).  Every case first
asserts in integers that its input reaches the branch it was built for, then asserts the call's full (all_ok, status) or (bytes, status) answer, stated beforehand, in both forms
of the verifier.  Every comparison is exact and nothing expected comes from the code under test.

  A  the weights of nbls_kzg_verify_cells: faults on elements, proofs and commitments that cancel in the plain sums are caught under every seed; faults built to cancel under
     the documented r_j are accepted with that seed, which pins r_j by the cell's position in s1, s2, s3 and in kzg_cell_interp_kernel<true> (two rounds of one lane group: the
     weight of the cell, not of the group), and caught under any other seed, the seed of the OS and after a rotation; A = B = O from non-zero members
  B  the zero flags of B's three parts with A zero or not, one row per combination (kzg_cells_adversarial_cases.MATRIX), at (8,3) and, for the rows about S, at (1,0); the two
     arms of the per-cell rule among good neighbours
  C  sizes: 16,400 cells at c = 64, where fr_cell_workgroups stops at FR_CELL_MAX_WG and a lane group walks five cells; the kernels indexed by cell past their first block;
     257 blobs at (8,3), where the proofs loop of cells_pipeline takes its natural second pass with one blob in it
  D  every lane of a cell as the offender of the canonical check of kzg_cell_interp_kernel; the borders of kzg_ntt_kernel's lanes in its cells mode
  E  recovery: a changed element and an element >= r in either half, at either end of a cell, in a lane's first and last slot, in the first and the last staged entry; a
     refused blob in first and in last place
  F  the three calls on one context in growing sizes: SB_KZGV_*, SB_KZGC_*, SB_KZGR_Z and SB_MSMB_* regrow between them

Oracle multiplications per module-scoped fixture: mono(log2_n) 2^log2_n (sizes 1, 2, 7, 8, 10; memoised in kzg_cells_cases for the whole run); world(8,3) 130 (two commitments,
every cell's proof); world(8,6) 18; world(2,1) 10; world(7,6) 4; matrix(shape) at most 80 (40 tuples of a commitment and a proof); tau_c one in G2 per cell size.  The tests
add at most a dozen each for their forged points, the (10,4) case of D2 128 for its neighbours' proofs."""
import hashlib
import importlib
import random
import pytest
from goldenio import hx
from kzg_cases import R, M256, NOT_VERIFIED, NON_CANONICAL, ZERO48, Setup, b32, blob_bytes, weight
from kzg_cells_cases import to_coeffs, cells, cell_proof, monomial_setup, rows
from kzg_verify_cells_cases import random_blob, cells_per_blob, with_element, bumped, LANES, WALK
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, recover
from kzg_cells_adversarial_cases import MATRIX, FORGED_ROWS, S_ROWS, Forge, values, call_args, matrix_rows

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
SEED2 = hashlib.sha256(b'kzg cells adversarial').digest()
MAX_WG = 1024          # FR_CELL_MAX_WG


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
def bad_points(golden):
    vec = golden['codec']['g1']
    return {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}


class World:
    """two random blobs of one shape and a pool of their honest (cell, proof) pairs as CellItems: one oracle multiplication per pooled proof, made once and left unchanged"""
    def __init__(self, setup, shape, seed, pool_per_blob):
        rnd = random.Random(seed)
        self.shape, self.fg, self.m = shape, Forge(setup, *shape), cells_per_blob(*shape)
        self.blobs = [random_blob(setup, *shape, rnd) for _ in range(2)]
        ks = [sorted(rnd.sample(range(self.m), min(pool_per_blob, self.m))) for _ in self.blobs]
        self.pool = [self.fg.honest(b, k) for b, kk in zip(self.blobs, ks) for k in kk]

    def draw(self, n, rnd):
        return [rnd.choice(self.pool) for _ in range(n)]


@pytest.fixture(scope='module')
def world(setup):
    """(log2_n, log2_cell) -> the World of that shape"""
    per = {(8, 3): 64, (8, 6): 8, (2, 1): 4, (7, 6): 4}
    made = {}

    def get(*shape):
        if shape not in made:
            made[shape] = World(setup, shape, 9300 + 16 * shape[0] + shape[1], per[shape])
        return made[shape]
    return get


@pytest.fixture(scope='module')
def ver(eng, mono, tau_c):
    """the verifier with this module's setup behind it: ver(shape, items or argument lists, seed, per_item)"""
    def run(shape, what, seed=SEED, per_item=True):
        cs, ci, ki, cl, pf = call_args(what) if not isinstance(what, tuple) else what
        return eng.kzg_verify_cells(mono(shape[0]), shape[1], cs, ci, ki, cl, pf, tau_c(shape[1]), seed, per_item)
    return run


def nines(n, at):
    return bytes(NOT_VERIFIED if j in at else 0 for j in range(n))


def check(ver, fg, items, bad, seeds=(SEED,)):
    """`bad`: the places that do not hold.  First the input itself, in integers -- which tuples hold, and what the combined check makes of them under a known seed (a weighted
    sum of the tuples' defects that is zero, or not) --, then the call's answer with statuses and the fast verdict"""
    bad, n = set(bad), len(items)
    assert {j for j, t in enumerate(items) if not fg.holds(t)} == bad
    for seed in seeds:
        if seed is not None:
            assert (fg.weighted_defect(items, seed, bad) == 0) == (not bad)
        assert ver(fg.shape, items, seed) == (not bad, nines(n, bad))
        assert ver(fg.shape, items, seed, per_item=False) == (not bad, None)


def accepted_though_wrong(ver, fg, items, bad):
    """the attack the NULL seed exists for: the tuples at `bad` do not hold, yet their weighted defects cancel under SEED, so the combined check NECESSARILY accepts with that
    seed -- that it does pins the documented r_j for the cells' positions in every sum they enter.  Any other seed, the seed of the OS and a rotation of the call reject"""
    n = len(items)
    assert {j for j, t in enumerate(items) if not fg.holds(t)} == set(bad)
    assert fg.weighted_defect(items, SEED, bad) == 0 and fg.weighted_defect(items, SEED2, bad) != 0
    assert ver(fg.shape, items, SEED) == (True, bytes(n))
    assert ver(fg.shape, items, SEED, per_item=False) == (True, None)
    for seed in (SEED2, None):
        assert ver(fg.shape, items, seed) == (False, nines(n, bad))
        assert ver(fg.shape, items, seed, per_item=False) == (False, None)


def launch_of(n, log2_cell):
    """fr_cell_workgroups and kzg_cell_interp_kernel's walk in the sum mode -> (workgroups, lane groups, rounds)"""
    per_wg = (LANES >> log2_cell) * WALK
    wg = min(-(-n // per_wg), MAX_WG)
    groups = wg * (LANES >> log2_cell)
    return wg, groups, -(-n // groups)


# ---- A. the weights

FAULTS = ['elements', 'proofs', 'commitments']


def pair_of(fg, rnd, k):
    """two free-form tuples at one cell index with a commitment each, which no other cell names"""
    return [fg.tuple_for(k, [rnd.randrange(R) for _ in range(fg.c)], rnd.randrange(2, R)) for _ in range(2)]


def faulted(fg, pair, fault, d, second, ja=2, jb=2):
    """the pair with an error worth d in the first tuple and `second` times d in the other: `second` = -1 cancels in the plain sums.  Elements: d is what is added to I(tau),
    through element ja of the first cell and element jb of the other (the Lagrange values at tau divide it out); proofs: to q (tau^c - s_k); commitments: to -cm"""
    ta, tb = pair
    e = d * second % R
    if fault == 'elements':
        return [fg.with_element(ta, ja, d * pow(fg.unit_at_tau(ta.k, ja), -1, R)), fg.with_element(tb, jb, e * pow(fg.unit_at_tau(tb.k, jb), -1, R))]
    if fault == 'proofs':
        return [fg.with_q(ta, ta.q + d * pow(fg.tau_c - fg.s(ta.k), -1, R)), fg.with_q(tb, tb.q + e * pow(fg.tau_c - fg.s(tb.k), -1, R))]
    return [fg.with_cm(ta, ta.cm - d), fg.with_cm(tb, tb.cm - e)]


@pytest.mark.parametrize('fault', FAULTS)
def test_cancellation_unweighted(ver, world, fault):
    """+d and -d in two cells of one cell index (the same element; the two proofs; the two commitments, each named by exactly one cell): the plain sums over the call are
    unchanged, so a check with weight 1 everywhere would accept.  With weights no seed does"""
    w, rnd = world(8, 3), random.Random(9400 + FAULTS.index(fault))
    fg = w.fg
    good = w.draw(6, rnd)
    pair = pair_of(fg, rnd, 37)
    bad = faulted(fg, pair, fault, rnd.randrange(1, R), -1)
    items = good[:1] + bad[:1] + good[1:4] + bad[1:] + good[4:]
    assert sum(fg.defect(t) for t in items) % R == 0          # the unweighted check
    if fault == 'elements':
        va, vb, v0, v1 = (values(t.cell_bytes) for t in bad + pair)
        assert [(x - y) % R for x, y in zip(va, v0)] == [(y - x) % R for x, y in zip(vb, v1)] and sum(x != y for x, y in zip(va, v0)) == 1          # +d and -d at one element
    elif fault == 'proofs':
        assert (bad[0].q + bad[1].q - pair[0].q - pair[1].q) % R == 0 and bad[0].q != pair[0].q
    else:
        assert (bad[0].cm + bad[1].cm - pair[0].cm - pair[1].cm) % R == 0 and [t.C for t in items].count(bad[0].C) == [t.C for t in items].count(bad[1].C) == 1
    check(ver, fg, items, {1, 5}, (SEED, SEED2, None))
    check(ver, fg, good[:1] + pair[:1] + good[1:4] + pair[1:] + good[4:], set(), (SEED, None))


# the places of the pair in a call of 300 cells at (8,3): 3 workgroups, 96 lane groups, 4 rounds
PLACES = {'one workgroup, round 0': (5, 9), 'two workgroups': (5, 40), 'one lane group, rounds 0 and 3': (5, 5 + 3 * 96)}


@pytest.mark.parametrize('place', sorted(PLACES))
@pytest.mark.parametrize('fault', FAULTS)
def test_cancellation_against_known_weights(ver, world, fault, place):
    """errors d and -d r_a / r_b at the places a and b of a call of 300 pooled cells.  The third placement puts both cells on ONE lane group of kzg_cell_interp_kernel<true>, in
    its rounds 0 and 3: the weight must be that of the cell (w32[kk]), not of the group (w32[q])"""
    a, b = PLACES[place]
    w, rnd = world(8, 3), random.Random(9410 + 16 * FAULTS.index(fault) + sorted(PLACES).index(place))
    fg = w.fg
    assert launch_of(300, 3) == (3, 96, 4)          # cell j: lane group j % 96 (32 groups a workgroup) in round j // 96
    same_workgroup, same_group, rounds = a % 96 // 32 == b % 96 // 32, a % 96 == b % 96, (a // 96, b // 96)
    assert (same_workgroup, same_group, rounds) == {'one workgroup, round 0': (True, False, (0, 0)), 'two workgroups': (False, False, (0, 0)),
                                                    'one lane group, rounds 0 and 3': (True, True, (0, 3))}[place]
    items = w.draw(300, rnd)
    pair = pair_of(fg, rnd, 11)
    ra, rb = weight(SEED, a), weight(SEED, b)
    items[a], items[b] = faulted(fg, pair, fault, rnd.randrange(1, R), -ra * pow(rb, -1, R), ja=2, jb=5)
    accepted_though_wrong(ver, fg, items, {a, b})
    moved = items[1:] + items[:1]
    check(ver, fg, moved, {a - 1, b - 1})
    items[a], items[b] = pair
    check(ver, fg, items, set())


def test_both_combined_points_zero_from_non_zero_members(ver, setup, matrix):
    """two valid tuples with r_0 q_0 + r_1 q_1 = 0: A is the zero point and, because valid tuples give B = tau^c A, so is B -- from three parts of B that are not.  Under another
    seed neither is zero.  After one element changes A is still zero and B is not"""
    fg, made = matrix(8, 3)
    items = made['none, A zero']
    assert fg.model(items, SEED) == ([False] * 3, True, True, True) and fg.model(items, SEED2) == ([False] * 3, False, False, True)
    check(ver, fg, items, set(), (SEED, SEED2, None))
    bad = made['none, A zero, B not']
    assert fg.model(bad, SEED) == ([False] * 3, True, False, False) and bad[1] == items[1] and bad[0].cell_bytes == bumped(items[0].cell_bytes, 0)
    check(ver, fg, bad, {0})


# ---- B. the zero-flag matrix

@pytest.fixture(scope='module')
def matrix(setup):
    """(log2_n, log2_cell) -> (the Forge of that shape, the rows of the zero-flag matrix under SEED)"""
    made = {}

    def get(*shape):
        if shape not in made:
            fg = Forge(setup, *shape)
            made[shape] = (fg, matrix_rows(fg, SEED, random.Random(9500 + shape[0])))
        return made[shape]
    return get


@pytest.mark.parametrize('shape,row', [((8, 3), name) for name in MATRIX] + [((1, 0), name) for name in S_ROWS])
def test_zero_flag_matrix(ver, matrix, shape, row):
    """(1,0): c = 1, kzg_cell_interp_kernel has no stage and the third part of B is one scalar against one point"""
    fg, made = matrix(*shape)
    items = made[row]
    flags, za, zb = MATRIX[row]
    assert fg.model(items, SEED) == (flags, za, zb, row not in FORGED_ROWS)
    assert all(ZERO48 not in (t.C, t.P) for t in items)
    bad = {j for j, t in enumerate(items) if not fg.holds(t)}
    assert bool(bad) == (row in FORGED_ROWS)
    check(ver, fg, items, bad)
    if not bad:          # valid tuples are accepted under every seed, whatever is zero under this one
        assert ver(shape, items, None) == (True, bytes(len(items)))


@pytest.mark.parametrize('shape', [(8, 3), (1, 0)])
def test_both_arms_of_the_per_cell_rule_among_good_neighbours(ver, setup, shape):
    """X_k = C - [I_k(tau)]G1 + [s_k]pi_k.  With a non-zero proof a zero X_k fails (the left side of the pairing equation is not one); with the zero proof the cell holds exactly
    when X_k is the zero point -- once it is, once it is not"""
    fg, rnd = Forge(setup, *shape), random.Random(9600 + shape[0])
    rv = lambda: rnd.randrange(2, R)
    cell = lambda: [rv() for _ in range(fg.c)]
    good = [fg.tuple_for(k, cell(), rv()) for k in (0, fg.m - 1, 1)]
    v, q = cell(), rv()
    x_zero = fg.item(fg.at_tau(2, v) - fg.s(2) * q, q, 2, v)          # cm - I + s q = 0 under q != 0
    zero_ok = fg.tuple_for(3, cell(), 0)                               # cm = I under q = 0
    zero_bad = fg.item(zero_ok.cm + rv(), 0, 3, values(zero_ok.cell_bytes))
    assert (x_zero.cm - x_zero.I + fg.s(2) * x_zero.q) % R == 0 and x_zero.P != ZERO48 and x_zero.C != ZERO48
    assert zero_ok.P == zero_bad.P == ZERO48 and zero_ok.cm == zero_ok.I and zero_bad.cm != zero_bad.I
    items = [good[0], x_zero, good[1], zero_bad, zero_ok, good[2]]
    check(ver, fg, items, {1, 3}, (SEED, None))
    check(ver, fg, [good[0], zero_ok, good[1]], set())


# ---- C. sizes

def test_sum_mode_at_its_workgroup_cap(ver, world):
    """16,400 cells at (8,6) from a pool of 16 (cell, proof) pairs: fr_cell_workgroups stops at 1024 workgroups, the 4096 lane groups walk five cells each and the fifth
    round holds 16 cells.  The per-cell pass behind a rejection is the rows mode with 4100 workgroups and msm_rows_dev with 16,400 rows"""
    n, shape = 16400, (8, 6)
    assert launch_of(n, 6) == (MAX_WG, 4096, 5) and launch_of(16384, 6) == (MAX_WG, 4096, 4) and n - 4 * 4096 == 16
    w, rnd = world(*shape), random.Random(9700)
    fg = w.fg
    assert len(w.pool) == 16
    items = w.draw(n, rnd)
    check(ver, fg, items, set())
    first = 4 * 4096          # the first cell of the fifth round
    bad = list(items)
    bad[first] = fg.with_element(bad[first], 63, 1)
    check(ver, fg, bad, {first})
    a, b = 5, 5 + 4 * 4096          # lane group 5 in its rounds 0 and 4
    pair = pair_of(fg, rnd, 3)
    bad = list(items)
    bad[a], bad[b] = faulted(fg, pair, 'elements', rnd.randrange(1, R), -weight(SEED, a) * pow(weight(SEED, b), -1, R), ja=0, jb=63)
    assert {j for j, t in enumerate(bad) if not fg.holds(t)} == {a, b}
    assert fg.weighted_defect(bad, SEED, {a, b}) == 0 and fg.weighted_defect(bad, SEED2, {a, b}) != 0
    assert ver(shape, bad, SEED) == (True, bytes(n))
    assert ver(shape, bad, SEED, per_item=False) == (True, None)
    assert ver(shape, bad, SEED2) == (False, nines(n, {a, b}))
    assert ver(shape, bad, SEED2, per_item=False) == (False, None)


def test_kernels_indexed_by_cell_past_their_first_block(ver, setup, world, bad_points):
    """600 pooled cells at (8,3): kzg_cell_pre_kernel and kzg_item_status_kernel (256 cells a block) and kzg_cell_items_kernel (64) meet every special cell in their later blocks"""
    shape, n = (8, 3), 600
    w, rnd = world(*shape), random.Random(9710)
    fg = w.fg
    items = w.draw(n, rnd)
    low = random_blob(setup, 8, 3, rnd, degree=8)          # degree < c: every quotient is zero, the commitment is not
    assert low.commitment != ZERO48
    for j, k in ((320, 5), (540, 63)):
        items[j] = fg.honest(low, k)
        assert items[j].P == ZERO48 and items[j].q == 0
    check(ver, fg, items, set())
    cs, ci, ki, cl, pf = call_args(items, extra_commitments=[bad_points['subgroup']])
    assert len(cs) == 4
    want = [0] * n
    for j in (300, 520):          # every cell that names the commitment outside the subgroup, and no other
        ci[j], want[j] = 3, 3
    pf[310], want[310] = bad_points['subgroup'], 13
    pf[530], want[530] = bad_points['noroot'], 14
    pf[330], want[330] = ZERO48, NOT_VERIFIED          # an ordinary cell with the zero proof
    assert items[330].q != 0
    cl[340], want[340] = with_element(cl[340], 7, R), NON_CANONICAL
    cl[599], want[599] = with_element(cl[599], 0, M256), NON_CANONICAL
    assert min(j for j, v in enumerate(want) if v) >= 256 and max(j for j, v in enumerate(want) if v) >= 512
    assert ver(shape, (cs, ci, ki, cl, pf)) == (False, bytes(want))
    assert ver(shape, (cs, ci, ki, cl, pf), per_item=False) == (False, None)
    assert ver(shape, (cs, ci, ki, cl, pf), None) == (False, bytes(want))


def test_natural_pass_boundary_of_the_proofs_loop(pkg, eng, setup, mono, world):
    """257 blobs at (8,3): a pass of the batched MSM takes 2^22 scalars, 2^14 rows of 256, the cells of 256 blobs -- the tail pass holds one blob, with a plan of its own.  Both
    front ends; the recovery has its three refused blobs at 0, 255 and 256, so that its tail pass is a refused blob alone.  The same input through passes of 100 blobs on a
    second engine gives the same bytes"""
    L, lc, m, n = 8, 3, 64, 257
    assert min(n, ((1 << 22) >> L) // m, (1 << 20) // m) == 256
    w, rnd = world(L, lc), random.Random(9720)
    cb = [[b.cell(k) for k in range(m)] for b in w.blobs]
    pf = [[b.proof(k) for k in range(m)] for b in w.blobs]
    which = [rnd.randrange(2) for _ in range(n - 2)] + [1, 0]
    blobs = [blob_bytes(w.blobs[x].f) for x in which]
    other = pkg.Engine(0)
    other.set_cells_chunk(100)
    got = eng.kzg_compute_cells_and_proofs(mono(L), lc, blobs)
    assert got[2] == bytes(n)
    assert got[0] == [cb[x] for x in which] and got[1] == [pf[x] for x in which]
    assert other.kzg_compute_cells_and_proofs(mono(L), lc, blobs) == got
    idxs = [rnd.sample(range(m), m // 2 + rnd.randrange(3)) for _ in range(n)]
    idxs[0], idxs[256] = idxs[0][:m // 2 - 1], rnd.sample(range(m), m // 2 + 1)
    given = [[cb[x][k] for k in idx] for x, idx in zip(which, idxs)]
    given[255][-1] = with_element(given[255][-1], 7, R)
    given[256][0] = bumped(given[256][0], 3)
    assert recover(idxs[256], [values(v) for v in given[256]], L, lc)[0] == INCONSISTENT
    want_st = bytes({0: BAD_CELLS, 255: NON_CANONICAL, 256: INCONSISTENT}.get(i, 0) for i in range(n))
    got = eng.kzg_recover_cells_and_proofs(mono(L), lc, idxs, given)
    assert got[2] == want_st
    assert got[0] == [[bytes(32 << lc)] * m if want_st[i] else cb[x] for i, x in enumerate(which)]
    assert got[1] == [[bytes(48)] * m if want_st[i] else pf[x] for i, x in enumerate(which)]
    assert other.kzg_recover_cells_and_proofs(mono(L), lc, idxs, given) == got
    other.close()


# ---- D. lane coverage of the canonical checks

@pytest.mark.parametrize('shape', [(2, 1), (8, 3), (7, 6)])
def test_every_lane_of_a_cell_refuses(ver, world, shape):
    """2 c + 1 cells; the odd places carry an element >= r, the j-th of them at element j: every lane of a cell is the offender once and must reach lane 0, which writes the
    status (for (m = 1; m < c; m <<= 1) bad |= shfl_xor(bad, m)), and no further: the even places are good cells on the neighbouring lanes of the same wavefront"""
    w, rnd = world(*shape), random.Random(9800 + shape[0])
    fg, c = w.fg, 1 << shape[1]
    n = 2 * c + 1
    items = w.draw(n, rnd)
    cs, ci, ki, cl, pf = call_args(items)
    for j in range(c):
        cl[2 * j + 1] = with_element(cl[2 * j + 1], j, (R, M256)[j % 2])
    want = bytes(NON_CANONICAL * (j % 2) for j in range(n))
    assert want.count(NON_CANONICAL) == c
    assert c == 64 or launch_of(n, shape[1])[2] == 1          # c < 64: one round, the cells lie side by side on the lanes of a wavefront in the order of the call
    for seed in (SEED, None):
        assert ver(shape, (cs, ci, ki, cl, pf), seed) == (False, want)
        assert ver(shape, (cs, ci, ki, cl, pf), seed, per_item=False) == (False, None)
    check(ver, fg, items, set())


@pytest.mark.parametrize('log2_n,log2_cell', [(10, 4), (12, 6)])
def test_ntt_cells_mode_refuses_at_every_lane_border(eng, setup, mono, log2_n, log2_cell):
    """kzg_ntt_kernel has 512 lanes a blob, lane t on the elements t, t + 512, ..: an element >= r in the first and the last lane's first and last slot, between good blobs"""
    rnd = random.Random(9810 + log2_n)
    n, m = 1 << log2_n, cells_per_blob(log2_n, log2_cell)
    f = [rnd.randrange(R) for _ in range(n)]
    good, at = blob_bytes(f), [0, 511, 512, n - 512, n - 1]
    blobs = [good]
    for j, i in enumerate(at):
        blobs += [good[:32 * i] + b32((R, M256)[j % 2]) + good[32 * i + 32:], good]
    want_cells = [rows(c) for c in cells(f, log2_n, log2_cell)]
    zero_cells = [bytes(32 << log2_cell)] * m
    want_st = bytes(NON_CANONICAL * (j % 2) for j in range(len(blobs)))
    got, st = eng.kzg_compute_cells(log2_n, log2_cell, blobs)
    assert st == want_st and got == [zero_cells if j % 2 else want_cells for j in range(len(blobs))]
    if log2_n == 10:
        coef = to_coeffs(f, log2_n)
        want_proofs = [cell_proof(setup, coef, k, log2_n, log2_cell) for k in range(m)]
        got, pf, st = eng.kzg_compute_cells_and_proofs(mono(log2_n), log2_cell, blobs)
        assert st == want_st and got == [zero_cells if j % 2 else want_cells for j in range(len(blobs))]
        assert pf == [[bytes(48)] * m if j % 2 else want_proofs for j in range(len(blobs))]


# ---- E. recovery: every element is looked at

def sweep(log2_n, log2_cell):
    """(cell, element, the changed cell is the first or the last staged entry): the first and the last cell of either half of the extension -- the lanes' first slots
    (i mod N < 512) and last slots (i mod N >= N - 512) --, either end of the cell, either end of the staged cells"""
    m, c = cells_per_blob(log2_n, log2_cell), 1 << log2_cell
    return [(k, e, last) for k in sorted({0, m // 2 - 1, m // 2, m - 1}) for e in sorted({0, c - 1}) for last in (False, True)]


@pytest.mark.parametrize('log2_n,log2_cell', [(5, 5), (8, 3), (10, 4), (11, 6), (12, 6)])
def test_recovery_looks_at_every_element(eng, setup, mono, world, log2_n, log2_cell):
    """Each changed blob is given M / 2 + 1 cells (both at (5,5)) of one polynomial with ONE element changed.  (M / 2 + 1) c - 1 >= N unchanged values already determine the
    polynomial of degree < N and the changed value contradicts it, so NBLS_ST_INCONSISTENT is the right answer without a reference run at the large shapes (up to (8,3) the
    specification's route in Python says so too); with the value r in that place the answer is NBLS_ST_NON_CANONICAL.  Every fourth blob is unchanged and comes back exact.

    What this pins: the canonical check reads both halves (dropping fr_recover_load(.., 1, ..) from it turns the 21 of the second half into 23), and a comparison with the given
    cells takes place (dropping both fr_recover_compare calls answers 0).  What NO input can pin is which of the two comparisons notices: with err the changes, W the
    interpolation of err Z over H u gH and W / Z = U + x^N V, the kernel's polynomial is P + U + 7^N V, which misses the given values by (7^N - 1) V on H and by (7^N + 1) V on
    gH.  The input contradicts itself exactly when V != 0, and deg V < (given cells - M / 2) c is below the number of given elements in EITHER half, so V cannot vanish on all of
    them: each comparison alone refuses exactly the inconsistent inputs, and dropping one of the two changes no answer of the call"""
    rnd = random.Random(9900 + 16 * log2_n + log2_cell)
    n, m, c = 1 << log2_n, cells_per_blob(log2_n, log2_cell), 1 << log2_cell
    proofs = (log2_n, log2_cell) == (8, 3)
    if proofs:
        blob = world(8, 3).blobs[0]
        ext, want_proofs = blob.cells, [blob.proof(k) for k in range(m)]
    else:
        ext = cells([rnd.randrange(R) for _ in range(n)], log2_n, log2_cell)
    cb = [rows(v) for v in ext]
    count = min(m // 2 + 1, m)
    assert count * c - 1 >= n
    cases = sweep(log2_n, log2_cell)
    assert {(k * c + e) % n < 512 for k, e, _ in cases} >= {True} and {(k * c + e) % n >= n - 512 for k, e, _ in cases} >= {True} and {k < m // 2 for k, _, _ in cases} == {True, False}
    idxs, plain, where = [], [], []          # where: per blob None, or (the staged entry, the element) that changes
    for j, (k, e, last) in enumerate(cases):
        if j % 3 == 0:
            idxs.append(rnd.sample(range(m), count)); plain.append([cb[x] for x in idxs[-1]]); where.append(None)
        others = rnd.sample([x for x in range(m) if x != k], count - 1)
        idxs.append(others + [k] if last else [k] + others)
        plain.append([cb[x] for x in idxs[-1]])
        where.append((count - 1 if last else 0, e))
    zero_cells = [bytes(32 * c)] * m
    for code, change in ((INCONSISTENT, lambda cell, e: bumped(cell, e)), (NON_CANONICAL, lambda cell, e: with_element(cell, e, R))):
        given = [list(g) for g in plain]
        for g, wh in zip(given, where):
            if wh is not None:
                g[wh[0]] = change(g[wh[0]], wh[1])
        if code == INCONSISTENT and log2_n <= 8:
            assert all(recover(idx, [values(v) for v in g], log2_n, log2_cell)[0] == INCONSISTENT for idx, g, wh in zip(idxs, given, where) if wh is not None)
        want_st = bytes(0 if wh is None else code for wh in where)
        want = [cb if wh is None else zero_cells for wh in where]
        if proofs:
            got, pf, st = eng.kzg_recover_cells_and_proofs(mono(log2_n), log2_cell, idxs, given)
            assert pf == [want_proofs if wh is None else [bytes(48)] * m for wh in where]
        else:
            got, st = eng.kzg_recover_cells(log2_n, log2_cell, idxs, given)
        assert st == want_st
        assert got == want


def test_refused_blob_first_and_last(eng):
    """a refused index set sends none of its cells: the staged cells then begin with another blob's (`if (!at) o_cells = o`), or end before the last blob's"""
    L, lc, m = 6, 2, 32
    rnd = random.Random(9950)
    exts = [[rows(v) for v in cells([rnd.randrange(R) for _ in range(1 << L)], L, lc)] for _ in range(3)]
    idxs = [rnd.sample(range(m), m // 2 + i) for i in range(3)]
    given = [[cb[k] for k in idx] for cb, idx in zip(exts, idxs)]
    short = rnd.sample(range(m), m // 2 - 1)
    refused = (short, [exts[0][k] for k in short])
    zero = [bytes(32 << lc)] * m
    got, st = eng.kzg_recover_cells(L, lc, [refused[0]] + idxs, [refused[1]] + given)
    assert (got, st) == ([zero] + exts, bytes([BAD_CELLS, 0, 0, 0]))
    got, st = eng.kzg_recover_cells(L, lc, idxs + [refused[0]], given + [refused[1]])
    assert (got, st) == (exts + [zero], bytes([0, 0, 0, BAD_CELLS]))
    got, st = eng.kzg_recover_cells(L, lc, [refused[0]] + idxs[:2] + [refused[0]], [refused[1]] + given[:2] + [refused[1]])
    assert (got, st) == ([zero] + exts[:2] + [zero], bytes([BAD_CELLS, 0, 0, BAD_CELLS]))
    nc = [with_element(given[0][0], 3, R)] + given[0][1:]
    got, st = eng.kzg_recover_cells(L, lc, idxs[:1] + idxs, [nc] + given)
    assert (got, st) == ([zero] + exts, bytes([NON_CANONICAL, 0, 0, 0]))


# ---- F. one context, three calls, growing sizes

def test_three_calls_on_one_context_in_growing_sizes(pkg, setup, tau_c, world):
    w, rnd = world(8, 3), random.Random(9960)
    fg, m = w.fg, 64
    cb = [[b.cell(k) for k in range(m)] for b in w.blobs]
    pf = [[b.proof(k) for k in range(m)] for b in w.blobs]
    five, big = w.draw(5, rnd), w.draw(600, rnd)
    big[444] = fg.with_element(big[444], 4, 1)
    assert all(fg.holds(t) for t in five) and {j for j, t in enumerate(big) if not fg.holds(t)} == {444}
    idx1 = rnd.sample(range(m), m // 2)
    idx5 = [rnd.sample(range(m), m // 2 + i) for i in range(5)]
    three = [1, 0, 1]
    poly = [[rnd.randrange(R) for _ in range(8)]]
    eng = pkg.Engine(0)          # every table and every slot of this context is made here
    mono = eng.kzg_monomial_setup(8, monomial_setup(setup, 8))
    verify = lambda items: eng.kzg_verify_cells(mono, 3, *call_args(items), tau_c(3), SEED)
    first = verify(five)
    assert first == (True, bytes(5))
    assert eng.kzg_recover_cells(8, 3, [idx1], [[cb[0][k] for k in idx1]]) == ([cb[0]], bytes(1))
    assert eng.kzg_compute_cells_and_proofs(mono, 3, [blob_bytes(w.blobs[x].f) for x in three]) == ([cb[x] for x in three], [pf[x] for x in three], bytes(3))
    assert verify(big) == (False, nines(600, {444}))          # the per-cell pass
    assert eng.kzg_recover_cells_and_proofs(mono, 3, idx5, [[cb[i % 2][k] for k in idx] for i, idx in enumerate(idx5)]) == ([cb[i % 2] for i in range(5)], [pf[i % 2] for i in range(5)], bytes(5))
    assert verify(five) == first
    got, st = eng.fr_ntt(3, poly, False)
    assert st == [0] and [int.from_bytes(v, 'big') for v in got[0]] == to_coeffs(poly[0], 3)
    mono.close()
    eng.close()
