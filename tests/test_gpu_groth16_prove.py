"""The Groth16 prover on the GPU (-m gpu): nbls_groth16_pk_create / nbls_groth16_prove against a test-only proving key whose trapdoor is known (groth16_prove_cases.py: every
query point is a known multiple of a generator, the expected proof three scalars and three oracle multiplications -- no polynomial arithmetic between the witness and the
expected bytes), end to end through the existing nbls_groth16_verify with the matching verifying key, and nbls_groth16_quotient against Python integers.  Bit-exact.  The
wiping is checked through the handle's accessor nbls_groth16_pk_wiped (Engine.groth16_pk_wiped), which reads the secret arrays back."""
import importlib
import random
import pytest
import torch  # noqa: F401
from goldenio import hx
from kzg_cases import R, M256, ZERO48, b32
from groth16_prove_cases import instance, family, quotient, ProvingKey, UNSATISFIED, NON_CANONICAL

pytestmark = pytest.mark.gpu
EDECODE = -5


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def engine_g1(eng, scalars):
    """[k]G1 compressed for many k != 0 by the existing nbls_g1_mul_batch on the generator and nbls_g1_compress_batch"""
    aff, st = eng.point_mul_batch([b32(k) for k in scalars])
    assert st == bytes(len(scalars))
    raw = eng.compress_batch(aff)
    return [raw[48 * i:48 * i + 48] for i in range(len(scalars))]


class Case:
    """an instance, its trapdoor key, the proving key on the device and the matching verifying key"""

    def __init__(self, eng, oracle, log2_n, n_vars, m, mats, seed, h_by_engine=False):
        self.rnd = random.Random(seed)
        self.log2_n, self.n_vars, self.m, self.mats = log2_n, n_vars, m, mats
        self.key = ProvingKey(oracle, log2_n, n_vars, m, mats, self.rnd)
        self.points = self.key.points(engine_g1(eng, self.key.h_scalars()) if h_by_engine else None)
        self.pk = eng.groth16_pk(log2_n, n_vars, m, mats, **self.points)
        self.vk = eng.groth16_vk(*self.key.vk_points())

    def rs(self):
        return self.rnd.randrange(R), self.rnd.randrange(R)


@pytest.fixture(scope='module')
def fam(eng, oracle):
    """N = 16: 8 free columns (column 5 named by no row), 11 rows, 19 variables, 3 public inputs; the variables the rows write have zero a_query / b_query points"""
    rnd = random.Random(1800)
    A, B, Cm, witness = family(4, 8, 11, rnd, skip=(5,))
    case = Case(eng, oracle, 4, 19, 3, (A, B, Cm), 1801)
    case.witness = witness
    return case


# ---- proof bytes

@pytest.mark.parametrize('shape', [(1, 4, 1, 0), (4, 20, 3, 0), (6, 70, 4, 3)], ids=str)
def test_proof_bytes(eng, oracle, shape):
    log2_n, n_vars, m, tail = shape
    rnd = random.Random(1810 + log2_n)
    A, B, Cm, z = instance(log2_n, n_vars, m, rnd)
    case = Case(eng, oracle, log2_n, n_vars, m, (A, B, Cm), 1820 + log2_n)
    assert (case.pk.log2_n, case.pk.n_vars, case.pk.n_public) == (log2_n, n_vars, m)
    eng.set_ntt_plan(tail_bits=tail, pass_bits=1 if tail else 0)
    try:
        pairs = [case.rs(), (0, 0), (R - 1, 1)]
        proofs, st = eng.groth16_prove(case.pk, [z] * 3, rs=pairs)
    finally:
        eng.set_ntt_plan(tail_bits=0, pass_bits=0)
    assert st == [0, 0, 0]
    for proof, (r, s) in zip(proofs, pairs):
        assert proof == case.key.expected_proof(z, r, s)
    assert eng.groth16_verify(case.vk, proofs, [z[1:m + 1]] * 3) == (True, bytes(3))


def test_proof_bytes_past_one_workgroups_transform(eng, oracle):
    """N = 2^13: the multi-pass transforms on the default plan; the 8191 h_query points by the existing nbls_g1_mul_batch on the generator"""
    rnd = random.Random(1830)
    A, B, Cm, z = instance(13, 300, 4, rnd)
    case = Case(eng, oracle, 13, 300, 4, (A, B, Cm), 1831, h_by_engine=True)
    r, s = case.rs()
    proofs, st = eng.groth16_prove(case.pk, [z], rs=[(r, s)])
    assert st == [0] and proofs[0] == case.key.expected_proof(z, r, s)


# ---- end to end

def test_five_witnesses_are_accepted_by_the_verifier(eng, fam):
    zs = [fam.witness(fam.rnd) for _ in range(5)]
    inputs = [z[1:fam.m + 1] for z in zs]
    pairs = [fam.rs() for _ in zs]
    proofs, st = eng.groth16_prove(fam.pk, zs, rs=pairs)
    assert st == [0] * 5 and proofs == [fam.key.expected_proof(z, r, s) for z, (r, s) in zip(zs, pairs)]
    assert eng.groth16_verify(fam.vk, proofs, inputs) == (True, bytes(5))
    # a proof does not verify for its neighbour's inputs
    assert eng.groth16_verify(fam.vk, proofs, inputs[1:] + inputs[:1])[0] is False
    # r and s from the OS: accepted, and never the same bytes twice
    first, st1 = eng.groth16_prove(fam.pk, zs)
    second, st2 = eng.groth16_prove(fam.pk, zs)
    assert st1 == [0] * 5 and st2 == [0] * 5
    assert eng.groth16_verify(fam.vk, first, inputs) == (True, bytes(5)) and eng.groth16_verify(fam.vk, second, inputs) == (True, bytes(5))
    assert len(set(first + second + proofs)) == 15


# ---- bad witnesses

def test_bad_witnesses_among_valid_neighbours(eng, fam):
    zs = [fam.witness(fam.rnd) for _ in range(7)]
    pairs = [fam.rs() for _ in zs]
    good, st = eng.groth16_prove(fam.pk, zs, rs=pairs)
    assert st == [0] * 7
    bad = [z[:] for z in zs]
    bad[1][-1] = (bad[1][-1] + 1) % R          # one violated row
    bad[3][0] = 0                              # z_0 = 0
    bad[5][2] = R                              # an element >= r
    proofs, st = eng.groth16_prove(fam.pk, bad, rs=pairs)
    assert st == [0, UNSATISFIED, 0, UNSATISFIED, 0, NON_CANONICAL, 0]
    for i in range(7):
        assert proofs[i] == (good[i] if st[i] == 0 else bytes(192)), i
    # r or s >= r, and a z_0 that is both non-canonical and not one
    pairs2 = [pairs[0], (R, 1), (1, M256)]
    proofs, st = eng.groth16_prove(fam.pk, [zs[0], zs[1], [R + 1] + zs[2][1:]], rs=pairs2)
    assert st == [0, NON_CANONICAL, NON_CANONICAL] and proofs == [good[0], bytes(192), bytes(192)]


# ---- masked queries and zero A

def test_masked_zero_query_points(eng, fam):
    """the family's key holds the zero point in a_query, b_g1_query and b_g2_query for every variable a row writes, and in l_query for the column no row names: their
    statuses are 1, the key is accepted, and the proofs are the expected bytes (test_five_witnesses..: the same key)"""
    nv, m = fam.n_vars, fam.m
    st = fam.pk.status
    assert len(st) == 5 + 3 * nv + (nv - m - 1) + 15 and st[:5] == bytes(5)
    aq, b1, b2, lq, hq = st[5:5 + nv], st[5 + nv:5 + 2 * nv], st[5 + 2 * nv:5 + 3 * nv], st[5 + 3 * nv:5 + 3 * nv + nv - m - 1], st[-15:]
    assert list(aq[8:]) == [1] * 11 and list(b1[8:]) == [1] * 11 and b1 == b2 and aq[5] == 1 and b1[5] == 1 and lq[5 - m - 1] == 1 and hq == bytes(15)
    assert fam.points['a_query48'][8] == ZERO48 and sum(lq) == 1 and 0 < sum(aq[:8]) + sum(b1[:8]) < 16
    z = fam.witness(fam.rnd)
    r, s = fam.rs()
    proofs, pst = eng.groth16_prove(fam.pk, [z], rs=[(r, s)])
    assert pst == [0] and proofs[0] == fam.key.expected_proof(z, r, s)


def test_zero_a_has_status_one(eng, fam):
    zs = [fam.witness(fam.rnd) for _ in range(3)]
    pairs = [fam.rs(), (fam.key.r_for_zero_a(zs[1]), 77), fam.rs()]
    proofs, st = eng.groth16_prove(fam.pk, zs, rs=pairs)
    assert st == [0, 1, 0] and proofs[1] == bytes(192)
    assert proofs[0] == fam.key.expected_proof(zs[0], *pairs[0]) and proofs[2] == fam.key.expected_proof(zs[2], *pairs[2])


# ---- the bytes depend on no tuning key

def test_row_wave_and_transform_plan_change_no_byte(eng, oracle):
    """rows of 1 .. 3 entries, two of 40 and one of 70 (the default threshold is 32): every threshold puts other rows on the wavefront path"""
    rnd = random.Random(1840)
    lengths = [(rnd.randrange(1, 4), rnd.randrange(1, 4)) for _ in range(40)] + [(40, 2), (3, 40), (70, 70)]
    A, B, Cm, z = instance(6, 72, 2, rnd, lengths=lengths)
    case = Case(eng, oracle, 6, 72, 2, (A, B, Cm), 1841)
    r, s = case.rs()
    want = case.key.expected_proof(z, r, s)
    try:
        for row_wave, tail, passes in ((0, 0, 0), (1, 0, 0), (8, 3, 1), (0, 2, 4), (64, 3, 2), (1 << 20, 0, 0)):
            eng.set_groth16_row_wave(row_wave)
            eng.set_ntt_plan(tail_bits=tail, pass_bits=passes)
            proofs, st = eng.groth16_prove(case.pk, [z], rs=[(r, s)])
            assert st == [0] and proofs[0] == want, (row_wave, tail, passes)
        # a violated long row is seen on either path
        k, v = Cm[-1][0]
        spoiled = Case(eng, oracle, 6, 72, 2, (A, B, Cm[:-1] + [[(k, (v + 1) % R)]]), 1842)
        for row_wave in (1, 1 << 20):
            eng.set_groth16_row_wave(row_wave)
            assert eng.groth16_prove(spoiled.pk, [z], rs=[(r, s)]) == ([bytes(192)], [UNSATISFIED])
    finally:
        eng.set_groth16_row_wave(0)
        eng.set_ntt_plan(tail_bits=0, pass_bits=0)


# ---- key refusals

def test_key_refusals(pkg, eng, fam, golden):
    g1 = golden['codec']['g1']
    off_subgroup = [hx(v['hex']) for v in g1 if 'subgroup' in v['result']][0]
    nv, m = fam.n_vars, fam.m
    base = 5 + 3 * nv + (nv - m - 1)          # where h_query's statuses start

    def refused(points):
        with pytest.raises(pkg.KzgSetupError) as e:
            eng.groth16_pk(fam.log2_n, nv, m, fam.mats, **points)
        assert e.value.code == EDECODE
        return e.value.status

    p = dict(fam.points)
    p['h_query48'] = p['h_query48'][:3] + [ZERO48] + p['h_query48'][4:]
    st = refused(p)
    assert st[base + 3] == 1 and sum(st[base:]) == 1 and st[:5] == bytes(5)          # the statuses are written all the same
    p = dict(fam.points, delta_g1_48=ZERO48)
    assert refused(p)[3] == 1
    p = dict(fam.points)
    p['a_query48'] = [off_subgroup] + p['a_query48'][1:]
    st = refused(p)
    assert st[5] >= 2 and st[:5] == bytes(5) and st[6:5 + nv] == fam.pk.status[6:5 + nv]
    p = dict(fam.points)
    p['l_query48'] = p['l_query48'][:-1] + [off_subgroup]
    assert refused(p)[base - 1] >= 2
    # the key itself is still accepted
    assert eng.groth16_pk(fam.log2_n, nv, m, fam.mats, **fam.points).n_vars == nv


# ---- the quotient alone

def triples(log2_n, seed):
    rnd, N = random.Random(seed), 1 << log2_n
    a = [[rnd.randrange(R) for _ in range(N)] for _ in range(3)]
    b = [[rnd.randrange(R) for _ in range(N)] for _ in range(3)]
    a[0][0], a[0][N - 1], b[0][N - 1], b[0][N // 2] = 0, R - 1, R - 1, 0
    return a, b, [[x * y % R for x, y in zip(ra, rb)] for ra, rb in zip(a, b)]


@pytest.mark.parametrize('log2_n', [1, 6, 13])
def test_quotient_against_python_integers(eng, log2_n):
    a, b, c = triples(log2_n, 1850 + log2_n)
    b[1][1] = R          # the middle row is non-canonical
    h, st = eng.groth16_quotient(log2_n, a, b, c)
    assert st == [0, NON_CANONICAL, 0] and h[1] == [0] * (1 << log2_n)
    for i in ((0, 2) if log2_n < 13 else (0,)):          # (one row of 2^13 in Python integers is enough: the three share every launch)
        assert h[i] == quotient(a[i], b[i], c[i], log2_n) and h[i][-1] == 0
    if log2_n == 6:
        c[2][5] = (c[2][5] + 1) % R
        eng.set_ntt_plan(tail_bits=3, pass_bits=2)
        try:
            h2, st = eng.groth16_quotient(log2_n, a, b, c)
        finally:
            eng.set_ntt_plan(tail_bits=0, pass_bits=0)
        assert st == [0, NON_CANONICAL, UNSATISFIED] and h2[:2] == h[:2]


# ---- the secrets are wiped

def test_the_handle_is_wiped_after_every_call(eng, fam):
    z = fam.witness(fam.rnd)
    assert eng.groth16_pk_wiped(fam.pk)          # (as created, and after every call of the tests above)
    for zs, pairs in (([z], [fam.rs()]), ([z, [2] + z[1:]], None), ([z[:3] + [M256] + z[4:]], [(1, R)])):
        eng.groth16_prove(fam.pk, zs, rs=pairs)
        assert eng.groth16_pk_wiped(fam.pk)
