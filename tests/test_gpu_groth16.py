"""Groth16 on the GPU (-m gpu): nbls_groth16_input_sums against Python integers, nbls_groth16_prepare_inputs against the oracle's multiples, nbls_groth16_vk_create and
nbls_groth16_verify against a test-only key whose trapdoor is known (groth16_cases.py: every point is a known multiple of a generator from the oracle, every proof valid by
construction), and the statuses of mixed batches against the single-proof equation evaluated through nbls_miller_product on points the test builds.  Nothing expected comes
from the calls under test."""
import ctypes as C
import importlib
import random
import pytest
import torch  # noqa: F401
from goldenio import hx
from groth16_cases import R, M256, ZERO48, ZERO96, NOT_VERIFIED, NON_CANONICAL, ST_G16_C, ROWS_WG, MAX_WG, ONE12, Key, input_sums, weight

pytestmark = pytest.mark.gpu
SEED = bytes(range(32, 64))
W64 = (1 << 64) - 1


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


class Case:
    """a key with m inputs on the device and n valid proofs for random inputs"""

    def __init__(self, eng, oracle, n, m, seed):
        self.rnd = random.Random(seed)
        self.key = Key(oracle, m, self.rnd)
        self.vk = eng.groth16_vk(*self.key.vk_points())
        self.xs = [[self.rnd.randrange(R) for _ in range(m)] for _ in range(n)]
        self.abc = [self.key.prove(x, self.rnd) for x in self.xs]

    def proofs(self, abc=None):
        return [self.key.proof_bytes(t) for t in (self.abc if abc is None else abc)]


_cases = {}


@pytest.fixture(scope='module')
def case(eng, oracle):
    def get(n, m):
        if (n, m) not in _cases:
            _cases[(n, m)] = Case(eng, oracle, n, m, 1700 + 100 * n + m)
        return _cases[(n, m)]
    yield get
    _cases.clear()


@pytest.fixture(scope='module')
def bad_points(golden):
    g1, g2 = golden['codec']['g1'], golden['codec']['g2']
    return {'g1_noroot': [hx(v['hex']) for v in g1 if v['result'] == 'Invalid compressed G1 point'][0], 'g1_subgroup': [hx(v['hex']) for v in g1 if 'subgroup' in v['result']][0],
            'g2_subgroup': [hx(v['hex']) for v in g2 if 'subgroup' in v['result']][0]}


# ---- (a) nbls_groth16_input_sums

def mixed(n, m, rnd):
    ws = [rnd.choice([1, 1 << 63, W64, rnd.randrange(1 << 64)]) for _ in range(n)]
    return [[rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(m)] for _ in range(n)], ws


@pytest.mark.parametrize('n,m', [(1, 1), (2, 2), (ROWS_WG - 1, 63), (ROWS_WG, 64), (ROWS_WG + 1, 65), (3 * ROWS_WG + 1, 129), (ROWS_WG + 1, 1), (5, 328)])
def test_input_sums_against_python_integers(eng, n, m):
    rows, ws = mixed(n, m, random.Random(2000 + 1000 * n + m))
    assert eng.groth16_input_sums(rows, ws) == input_sums(rows, ws)


def test_input_sums_all_r_minus_1(eng):
    """the largest products, (2^64 - 1)(r - 1), in every lane's accumulator; the second shape has more rows than 1024 workgroups of 64, so that a row group walks further"""
    for n, m in ((3 * ROWS_WG + 1, 65), (MAX_WG * ROWS_WG + ROWS_WG + 1, 1)):
        rows, ws = [[R - 1] * m] * n, [W64] * n
        assert eng.groth16_input_sums(rows, ws) == ([n * W64 % R] + [n * W64 * (R - 1) % R] * m, [0] * n), (n, m)


def test_input_sums_rows_that_are_out(eng):
    n, m = ROWS_WG + 1, 65
    rows, ws = mixed(n, m, random.Random(2100))
    pre = [0] * n
    pre[3], pre[n - 1] = 13, 4
    rows[0][m - 1], rows[n // 2][0], rows[3][5] = R, M256, R
    got = eng.groth16_input_sums(rows, ws, pre)
    assert got == input_sums(rows, ws, pre)
    assert [i for i, s in enumerate(got[1]) if s] == [0, 3, n // 2, n - 1] and got[1][0] == got[1][n // 2] == NON_CANONICAL and got[1][3] == 13
    assert eng.groth16_input_sums(rows, ws)[0] == input_sums(rows, ws)[0]          # pre == NULL


# ---- (b) nbls_groth16_prepare_inputs

@pytest.mark.parametrize('n,m', [(1, 1), (5, 1), (1, 3), (5, 3), (1, 65), (5, 65)])
def test_prepare_inputs_against_the_oracle(eng, case, n, m):
    c = case(5, m)
    rows = [list(x) for x in c.xs[:n]]
    rows[0] = c.key.inputs_for_zero_l(c.rnd)          # L is the zero point
    if n > 1:
        rows[2][m - 1] = R                            # a non-canonical row
        rows[3] = [0] * m                             # L = IC_0
    pts, st = eng.groth16_prepare_inputs(c.vk, rows)
    for i, row in enumerate(rows):
        if any(x >= R for x in row):
            assert (pts[i], st[i]) == (bytes(48), NON_CANONICAL), i
        elif c.key.l_scalar(row) == 0:
            assert (pts[i], st[i]) == (ZERO48, 1), i
        else:
            assert (pts[i], st[i]) == (c.key.g1(c.key.l_scalar(row)), 0), i


# ---- (c) nbls_groth16_verify

@pytest.mark.parametrize('n,m', [(1, 1), (2, 3), (3, 65), (65, 2)])
def test_valid_batches_are_accepted(eng, case, n, m):
    c = case(n, m)
    for seed in (SEED, None):
        assert eng.groth16_verify(c.vk, c.proofs(), c.xs, seed=seed) == (True, bytes(n))
        assert eng.groth16_verify(c.vk, c.proofs(), c.xs, seed=seed, per_item=False) == (True, None)


def rejected(eng, c, proofs, xs, want):
    assert eng.groth16_verify(c.vk, proofs, xs, seed=SEED) == (False, bytes(want))
    assert eng.groth16_verify(c.vk, proofs, xs) == (False, bytes(want))
    assert eng.groth16_verify(c.vk, proofs, xs, seed=SEED, per_item=False) == (False, None)


def test_wrong_input_swapped_a_and_shifted_c(eng, case):
    c = case(3, 65)
    xs = [list(x) for x in c.xs]
    xs[1][64] = (xs[1][64] + 1) % R
    rejected(eng, c, c.proofs(), xs, [0, NOT_VERIFIED, 0])
    (a0, b0, c0), (a1, b1, c1), p2 = c.abc
    rejected(eng, c, c.proofs([(a1, b0, c0), (a0, b1, c1), p2]), c.xs, [NOT_VERIFIED, NOT_VERIFIED, 0])
    d = 0x1234567          # (C_0 + D, C_1 - D): an unweighted sum would accept
    rejected(eng, c, c.proofs([(a0, b0, (c0 + d) % R), (a1, b1, (c1 - d) % R), p2]), c.xs, [NOT_VERIFIED, NOT_VERIFIED, 0])


def test_malformed_proofs_get_the_statuses_the_header_states(eng, case, bad_points):
    c = case(9, 4)
    n = 8
    proofs, xs = c.proofs()[:n], [list(x) for x in c.xs[:n]]
    A, B, Cc = (lambda p: p[:48]), (lambda p: p[48:144]), (lambda p: p[144:])
    want = [0] * n
    proofs[0] = ZERO48 + B(proofs[0]) + Cc(proofs[0]); want[0] = 1
    proofs[1] = A(proofs[1]) + ZERO96 + Cc(proofs[1]); want[1] = 11
    proofs[2] = A(proofs[2]) + B(proofs[2]) + ZERO48; want[2] = ST_G16_C + 1
    proofs[3] = A(proofs[3]) + bad_points['g2_subgroup'] + Cc(proofs[3]); want[3] = 13
    proofs[4] = bad_points['g1_noroot'] + B(proofs[4]) + Cc(proofs[4]); want[4] = 4
    proofs[5] = A(proofs[5]) + B(proofs[5]) + bad_points['g1_subgroup']; want[5] = ST_G16_C + 3
    xs[6][0] = R; want[6] = NON_CANONICAL
    rejected(eng, c, proofs, xs, want)          # proof 7 is untouched: a neighbour is never disturbed
    # one at a time, and the order of the header where several apply
    for i in range(7):
        p1, x1 = c.proofs()[:n], [list(x) for x in c.xs[:n]]
        p1[i], x1[i] = proofs[i], xs[i]
        rejected(eng, c, p1, x1, [want[k] if k == i else 0 for k in range(n)])
    p1, x1 = c.proofs()[:n], [list(x) for x in c.xs[:n]]
    p1[2] = ZERO48 + bad_points['g2_subgroup'] + bad_points['g1_noroot']; x1[2][1] = M256
    p1[4] = A(p1[4]) + ZERO96 + bad_points['g1_noroot']; x1[4][0] = R
    p1[5] = A(p1[5]) + B(p1[5]) + bad_points['g1_noroot']; x1[5][0] = R
    rejected(eng, c, p1, x1, [0, 0, 1, 0, 11, ST_G16_C + 4, 0, 0])


def test_cancellation_against_known_weights(eng, case):
    """the weights are the stated function of the seed and the proof's position: (C_i + [r_j]D, C_j - [r_i]D) leaves sum_k [r_k]C_k as it was, so under THAT seed the combined
    check accepts the two spoiled proofs; under any other seed, and from the OS, they are found"""
    c = case(3, 65)
    d = 0x7654321
    for i, j in ((0, 1), (2, 0)):
        ri, rj = weight(SEED, i), weight(SEED, j)
        abc = list(c.abc)
        abc[i] = (abc[i][0], abc[i][1], (abc[i][2] + rj * d) % R)
        abc[j] = (abc[j][0], abc[j][1], (abc[j][2] - ri * d) % R)
        assert not c.key.holds_scalars(abc[i], c.xs[i]) and not c.key.holds_scalars(abc[j], c.xs[j])
        assert eng.groth16_verify(c.vk, c.proofs(abc), c.xs, seed=SEED) == (True, bytes(3))
        want = bytes(NOT_VERIFIED if k in (i, j) else 0 for k in range(3))
        assert eng.groth16_verify(c.vk, c.proofs(abc), c.xs, seed=bytes(32)) == (False, want)
        assert eng.groth16_verify(c.vk, c.proofs(abc), c.xs) == (False, want)


def test_acceptance_is_not_byte_based(eng, case):
    c = case(2, 3)
    (a, b, cc), other = c.abc
    half = pow(2, -1, R)
    assert eng.groth16_verify(c.vk, c.proofs([(2 * a % R, b * half % R, cc), other]), c.xs, seed=SEED) == (True, bytes(2))
    assert eng.groth16_verify(c.vk, c.proofs([(a, b, cc), (a, b, cc)]), [c.xs[0], c.xs[0]], seed=SEED) == (True, bytes(2))          # the same proof twice


def test_per_proof_pass_with_a_zero_l(eng, case):
    c = case(2, 3)
    x0 = c.key.inputs_for_zero_l(c.rnd)
    good = c.key.prove(x0, c.rnd)
    bad = (good[0], good[1], (good[2] + 1) % R)
    xs = [x0, c.xs[0], x0]
    assert eng.groth16_verify(c.vk, c.proofs([good, c.abc[0], good]), xs, seed=SEED) == (True, bytes(3))
    rejected(eng, c, c.proofs([good, c.abc[0], bad]), xs, [0, 0, NOT_VERIFIED])
    # every L the zero point and nothing else in the call: the combined point sum_j [S_j]IC_j is then the zero point too, the combined check does not count, and the per-proof
    # pass accepts what holds
    assert eng.groth16_verify(c.vk, c.proofs([good, good]), [x0, x0], seed=SEED) == (True, bytes(2))
    assert eng.groth16_verify(c.vk, c.proofs([good, bad]), [x0, x0], seed=SEED) == (False, bytes([0, NOT_VERIFIED]))


def test_chunks_do_not_change_a_byte(eng, case):
    c = case(5, 3)
    proofs, xs = c.proofs(), [list(x) for x in c.xs]
    xs[1][0] = (xs[1][0] + 1) % R
    xs[4][2] = R
    proofs[3] = proofs[3][:144] + ZERO48
    rows = [list(x) for x in xs]
    rows[0] = c.key.inputs_for_zero_l(c.rnd)
    want = [0, NOT_VERIFIED, 0, ST_G16_C + 1, NON_CANONICAL]
    ref_pts = eng.groth16_prepare_inputs(c.vk, rows)
    try:
        for chunk in (1, 2, 0):
            eng.set_groth16_chunk(chunk)
            assert eng.groth16_verify(c.vk, proofs, xs, seed=SEED) == (False, bytes(want)), chunk
            assert eng.groth16_prepare_inputs(c.vk, rows) == ref_pts, chunk
    finally:
        eng.set_groth16_chunk(0)
    assert ref_pts[1] == [1, 0, 0, 0, NON_CANONICAL]


# ---- (d) the key

def test_key_creation_refuses_bad_entries(pkg, eng, case, bad_points):
    c = case(2, 3)
    alpha, beta, gamma, delta, ic = c.key.vk_points()
    assert c.vk.inputs == 3
    for pos, zero, undec in [(0, ZERO48, bad_points['g1_noroot']), (1, ZERO96, bad_points['g2_subgroup']), (2, ZERO96, bad_points['g2_subgroup']), (3, ZERO96, bad_points['g2_subgroup']),
                             (4, ZERO48, bad_points['g1_subgroup']), (5, ZERO48, bad_points['g1_noroot']), (6, ZERO48, bad_points['g1_subgroup']), (7, ZERO48, bad_points['g1_noroot'])]:
        for pt, code in ((zero, 1), (undec, None)):
            args = [alpha, beta, gamma, delta] + list(ic)
            args[pos] = pt
            with pytest.raises(pkg.KzgSetupError) as e:
                eng.groth16_vk(args[0], args[1], args[2], args[3], args[4:])
            st = list(e.value.status)
            assert e.value.code == -5 and [i for i, s in enumerate(st) if s] == [pos] and (code is None or st[pos] == code) and st[pos] in (1, 3, 4), (pos, st)
    # *out = NULL
    lib, h = eng.lib, C.c_void_p(7)
    assert lib.nbls_groth16_vk_create(eng.h, 3, ZERO48, beta, gamma, delta, b''.join(ic), None, C.byref(h)) == -5 and h.value is None


def test_a_key_outlives_its_creating_context(pkg, oracle):
    first = pkg.Engine(0)
    rnd = random.Random(1800)
    key = Key(oracle, 2, rnd)
    vk = first.groth16_vk(*key.vk_points())
    xs = [[rnd.randrange(R) for _ in range(2)] for _ in range(2)]
    abc = [key.prove(x, rnd) for x in xs]
    first.close()
    second = pkg.Engine(0)
    assert second.groth16_verify(vk, [key.proof_bytes(t) for t in abc], xs) == (True, bytes(2))
    xs[1][0] = (xs[1][0] + 1) % R
    assert second.groth16_verify(vk, [key.proof_bytes(t) for t in abc], xs) == (False, bytes([0, NOT_VERIFIED]))
    vk.close()
    second.close()


# ---- (e) agreement with the single-proof equation through nbls_miller_product

def equation_holds(eng, key, abc, x):
    """e(A, B) e(L, -gamma) e(C, -delta) e(alpha, -beta) == 1 through the existing product call, on affine points built here; a zero L is a factor of one"""
    a, b, c = abc
    g1s, g2s = [key.g1_aff(a), key.g1_aff(c), key.g1_aff(key.alpha)], [key.g2_aff(b), key.g2_aff(-key.delta), key.g2_aff(-key.beta)]
    l = key.l_scalar(x)
    if l:
        g1s.append(key.g1_aff(l)); g2s.append(key.g2_aff(-key.gamma))
    return eng.miller_product(b''.join(g1s), b''.join(g2s), True)[0] == ONE12


def test_mixed_batches_agree_with_the_single_proof_equation(eng, case):
    c = case(9, 4)
    rnd = random.Random(1900)
    for batch in range(8):
        abc, xs = list(c.abc), [list(x) for x in c.xs]
        for i in rnd.sample(range(9), rnd.randrange(4)):
            kind = rnd.randrange(3)
            if kind == 0:
                xs[i][rnd.randrange(4)] = rnd.randrange(R)
            elif kind == 1:
                abc[i] = (abc[i][0], abc[i][1], rnd.randrange(1, R))
            else:
                abc[i] = (abc[(i + 1) % 9][0], abc[i][1], abc[i][2])
        want = [0 if equation_holds(eng, c.key, t, x) else NOT_VERIFIED for t, x in zip(abc, xs)]
        assert [0 if c.key.holds_scalars(t, x) else NOT_VERIFIED for t, x in zip(abc, xs)] == want
        ok, st = eng.groth16_verify(c.vk, c.proofs(abc), xs, seed=bytes([batch]) * 32)
        assert list(st) == want and ok == (not any(want)), batch
