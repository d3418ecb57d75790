"""Commitment polynomials evaluated on the GPU (-m gpu): nbls_g1_poly_eval / nbls_g2_poly_eval against the oracle.  f is a Python-integer polynomial mod r, the commitments are
oracle.get_public_key(a_j) (G1) and the compressed oracle.g2_mul(G2, a_j) (G2), the expected evaluation is the same with f(x mod r): nothing expected comes from the call under
test.  Mixed groups in one call in both forms of the Horner step (identifiers 1 .. m: 16 bits; random 256-bit identifiers), the identifier edges, zeros of the polynomial, zero
and undecodable coefficients, offsets, slabs, a polynomial of 4096 coefficients, the tie to combine_shares, the whole threshold flow, and the kernels in use.  Bit-exact."""
import ctypes as C
import importlib
import os
import random
import subprocess
import sys
import pytest
from goldenio import hx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M256 = (1 << 256) - 1
ZERO = {False: b'\xc0' + bytes(47), True: b'\xc0' + bytes(95)}
SHAPES = [(1, 1), (2, 1), (1, 3), (3, 5), (9, 17), (17, 15), (5, 16), (4, 65)]          # (t, m): t = 1 beside t = 17, the 8- and 16-item wavefront edges of the point programs
SIDES = [False, True]


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def b32(v):
    return v.to_bytes(32, 'big')


def f_at(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * (x % R) + c) % R
    return acc


class Side:
    """[k]G as compressed bytes from the oracle, G1 or G2; k = 0: the zero point's encoding"""
    def __init__(self, eng, oracle, g2):
        self.eng, self.oracle, self.g2, self.e, self.memo = eng, oracle, g2, 96 if g2 else 48, {}

    def points(self, ks):
        ks = [k % R for k in ks]
        new = sorted(set(k for k in ks if k and k not in self.memo))
        if self.g2 and new:          # the oracle has no G2 compression of its own: the engine's compress_batch (pinned to the reference's vectors by its own tests) on the oracle's points
            comp = self.eng.compress_batch(b''.join(self.oracle.g2_mul(self.oracle.g2_generator(), k)[1] for k in new), g2=True)
            self.memo.update((k, comp[96 * i:96 * i + 96]) for i, k in enumerate(new))
        for k in ([] if self.g2 else new):
            self.memo[k] = self.oracle.get_public_key(b32(k))
        return [self.memo[k] if k else ZERO[self.g2] for k in ks]

    def expected(self, coef, ids):
        s = [f_at(coef, x) for x in ids]
        return self.points(s), [0 if v else 1 for v in s]


@pytest.fixture(scope='module')
def sides(eng, oracle):
    return {g2: Side(eng, oracle, g2) for g2 in SIDES}


def check(eng, side, polys, idsets, **kw):
    """one call over the groups (coefficient lists as integers, identifier lists) against the oracle"""
    got, st = eng.poly_eval([(side.points(c), i) for c, i in zip(polys, idsets)], g2=side.g2, **kw)
    for g, (c, i) in enumerate(zip(polys, idsets)):
        want, wst = side.expected(c, i)
        assert st[g] == wst, (g, len(c), len(i))
        assert got[g] == want, (g, len(c), len(i))
    return got, st


# ---- oracle parity

@pytest.mark.parametrize('g2', SIDES)
@pytest.mark.parametrize('form', ['short', 'full'])
def test_mixed_groups_against_the_oracle(eng, sides, g2, form):
    rnd = random.Random(31 + g2)
    shapes = list(SHAPES)
    rnd.shuffle(shapes)
    polys = [[rnd.randrange(1, R) for _ in range(t)] for t, _ in shapes]
    idsets = [list(range(1, m + 1)) if form == 'short' else [rnd.getrandbits(256) for _ in range(m)] for _, m in shapes]
    check(eng, sides[g2], polys, idsets)


@pytest.mark.parametrize('g2', SIDES)
def test_identifier_edges(eng, sides, g2):
    side = sides[g2]
    rnd = random.Random(4)
    coef = [rnd.randrange(1, R) for _ in range(4)]
    ids = [0, 1, (1 << 16) - 1, 1 << 16, 1 << 64, R - 1, R, R + 1, M256]
    got, st = check(eng, side, [coef], [ids])
    a0 = side.points([coef[0]])[0]
    assert got[0][0] == a0 and got[0][6] == a0 and got[0][1] == got[0][7]          # F(0) = F(r) = A_0; x and x + r give equal bytes
    # identifiers below 2^16 alone take the short form: the same bytes
    small, _ = check(eng, side, [coef], [ids[:3]])
    assert small[0] == got[0][:3]


# ---- zero points

@pytest.mark.parametrize('g2', SIDES)
def test_zeros_of_the_polynomial_and_zero_coefficients(eng, sides, g2):
    side = sides[g2]
    rnd = random.Random(35)

    def times(p, q):
        out = [0] * (len(p) + len(q) - 1)
        for i, a in enumerate(p):
            for j, b in enumerate(q):
                out[i + j] = (out[i + j] + a * b) % R
        return out

    g = [rnd.randrange(1, R) for _ in range(3)]
    f = times(times([-3 % R, 1], [-5 % R, 1]), g)          # (x - 3)(x - 5) g(x)
    a = rnd.randrange(1, R)
    polys = [f, [a, a + 1, 0], [a, 0, 0, a + 2], [0, 0, 0], [0], [3, 1], [0, 0, a]]          # ..., a leading zero, a middle zero, all zero, A_0 = [3]G and A_1 = G
    idsets = [[1, 2, 3, 4, 5, 6], [1, 2, 9], [1, 7], [1, 2, M256], [5], [3, 1, R - 3], [0, 1, 2]]
    got, st = check(eng, side, polys, idsets)
    assert st[0] == [0, 0, 1, 0, 1, 0] and got[0][2] == got[0][4] == ZERO[g2]
    assert st[3] == [1, 1, 1] and st[4] == [1]
    assert st[5] == [0, 0, 1]          # at x = 3 equal points meet in the last addition; at x = -3 opposite ones
    assert got[5][0] == side.points([6])[0]
    assert st[6] == [1, 0, 0]


# ---- a coefficient that does not decode

@pytest.mark.parametrize('g2', SIDES)
def test_bad_coefficients_leave_the_neighbours_alone(eng, sides, golden, g2):
    side = sides[g2]
    rnd = random.Random(36)
    vec = golden['codec']['g2' if g2 else 'g1']
    sub = [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0]
    noroot = [hx(v['hex']) for v in vec if v['result'] == ('Failed to find a square root' if g2 else 'Invalid compressed G1 point')][0]
    shapes = [(3, 4), (5, 3), (2, 9), (7, 5), (4, 2), (9, 17), (3, 3), (2, 2)]
    polys = [[rnd.randrange(1, R) for _ in range(t)] for t, _ in shapes]
    polys[7] = [0, 0]                  # the zero polynomial: status 1 and 0xc0 00.. beside the statuses >= 2 and their all-zero bytes, in one call
    idsets = [[rnd.getrandbits(256) for _ in range(m)] for _, m in shapes]
    groups = [(side.points(c), i) for c, i in zip(polys, idsets)]
    bad = [(list(c), i) for c, i in groups]
    bad[1][0][2] = sub                 # outside the subgroup, in the middle of group 1
    bad[3][0][3] = noroot              # no square root, in the middle of group 3
    bad[5][0][4] = noroot              # two bad coefficients in one group: the first one's status
    bad[5][0][7] = sub
    got, st = eng.poly_eval(bad, g2=g2)
    clean, cst = eng.poly_eval([grp for g, grp in enumerate(groups) if g not in (1, 3, 5)], g2=g2)
    want = {1: 3, 3: 4, 5: 4}
    k = 0
    for g, (t, m) in enumerate(shapes):
        if g in want:
            assert st[g] == [want[g]] * m and got[g] == [bytes(side.e)] * m, g
        else:
            pts, wst = side.expected(polys[g], idsets[g])
            assert wst == ([1] if g == 7 else [0]) * m and st[g] == wst == cst[k] and got[g] == clean[k] == pts, g
            k += 1
    # the other order in one group
    bad[5][0][4], bad[5][0][7] = sub, noroot
    got, st = eng.poly_eval(bad[4:], g2=g2)
    assert st[1] == [3] * 17 and st[0] == [0] * 2 and st[2] == [0] * 3 and got[0] == clean[2]


# ---- offsets, slabs, a long polynomial

@pytest.mark.parametrize('g2', SIDES)
def test_offsets_need_not_start_at_zero(eng, sides, g2):
    side = sides[g2]
    rnd = random.Random(37)
    polys = [[rnd.randrange(1, R) for _ in range(t)] for t in (3, 2)]
    idsets = [[rnd.getrandbits(256) for _ in range(4)], [1, 2, 3]]
    e = side.e
    # two poisoned coefficients and three poisoned identifiers in front: never read
    coefs = b'\xff' * (2 * e) + b''.join(side.points(polys[0]) + side.points(polys[1]))
    ids = b'\xee' * (3 * 32) + b''.join(b32(x) for i in idsets for x in i)
    out, st = C.create_string_buffer(7 * e), C.create_string_buffer(b'\x55' * 7, 7)
    f = eng.lib.nbls_g2_poly_eval if g2 else eng.lib.nbls_g1_poly_eval
    assert f(eng.h, 2, (C.c_uint32 * 3)(2, 5, 7), coefs, (C.c_uint32 * 3)(3, 7, 10), ids, out, st) == 0
    want = side.expected(polys[0], idsets[0])[0] + side.expected(polys[1], idsets[1])[0]
    assert [out.raw[e * k:e * k + e] for k in range(7)] == want and st.raw == bytes(7)
    assert f(eng.h, 2, (C.c_uint32 * 3)(2, 5, 7), coefs, (C.c_uint32 * 3)(3, 7, 10), ids, out, None) == 0          # the statuses may be left out


@pytest.mark.parametrize('g2', SIDES)
def test_slabs(eng, sides, g2):
    """50 identifiers in three groups through slabs of 16: the second group straddles two slab edges, the last slab is short"""
    side = sides[g2]
    rnd = random.Random(38)
    polys = [[rnd.randrange(1, R) for _ in range(t)] for t in (3, 5, 2)]
    idsets = [[rnd.getrandbits(256) for _ in range(m)] for m in (13, 27, 10)]
    whole, _ = eng.poly_eval([(side.points(c), i) for c, i in zip(polys, idsets)], g2=g2)
    eng.set_poly_slab(16)
    try:
        cut, _ = check(eng, side, polys, idsets)
    finally:
        eng.set_poly_slab(0)
    assert cut == whole


def test_long_polynomial(eng, sides):
    """t = 4096 at the identifiers 1 .. 3: 4095 steps of the short form"""
    rnd = random.Random(4096)
    coef = [rnd.randrange(1, R) for _ in range(4096)]
    check(eng, sides[False], [coef], [[1, 2, 3]])


# ---- the tie to the merged calls

def test_lagrange_of_the_evaluation_is_the_constant_term(eng, sides):
    side = sides[False]
    rnd = random.Random(39)
    polys = [[rnd.randrange(1, R) for _ in range(t)] for t in (1, 2, 7, 67)]
    idsets = [[rnd.getrandbits(256) for _ in c] for c in polys]
    groups = [(side.points(c), i) for c, i in zip(polys, idsets)]
    pks, st = eng.poly_eval(groups)
    assert all(s == [0] * len(s) for s in st)
    back, st = eng.combine_shares([(i, p) for i, p in zip(idsets, pks)], g2=False)
    assert st == [0] * 4 and back == [c[0] for c, _ in groups]


def test_the_whole_threshold_flow(eng, oracle, sides):
    """split a key (3 of 5), commit, share keys from the commitment, verify the partial signatures under them, combine any three, verify under A_0"""
    rnd = random.Random(40)
    coef = [rnd.randrange(1, R) for _ in range(3)]
    ids = [1, 2, 3, 4, 5]
    msg = b'the whole flow'
    commitment = sides[False].points(coef)
    partial = [oracle.sign(msg, b32(f_at(coef, x)))[1] for x in ids]
    (share_keys,), _ = eng.poly_eval([(commitment, ids)])
    assert share_keys == [oracle.get_public_key(b32(f_at(coef, x))) for x in ids]
    ok, st = eng.verify_multiple_shared(partial, [msg], [0] * 5, share_keys)
    assert ok and not any(st)
    swapped = [partial[1], partial[0]] + partial[2:]
    ok, st = eng.verify_multiple_shared(swapped, [msg], [0] * 5, share_keys)
    assert not ok and st[0] and st[1] and not any(st[2:])
    for pick in ([0, 1, 2], [4, 2, 1], [3, 0, 4]):
        (sig,), st = eng.combine_shares([([ids[k] for k in pick], [partial[k] for k in pick])])
        assert st == [0] and sig == oracle.sign(msg, b32(coef[0]))[1]
        assert oracle.verify(sig, msg, commitment[0]) == 1


def test_other_calls_still_match_afterwards(eng, oracle, sides):
    """the new scratch slots collide with nothing: one combine_shares and one verify_multiple call give what they gave before calls of the new kind in both groups"""
    rnd = random.Random(41)
    coef = [rnd.randrange(1, R) for _ in range(3)]
    ids = [rnd.getrandbits(256) for _ in range(3)]
    keys = [b32(f_at(coef, x)) for x in ids]
    msgs = [b'neighbour %d' % i for i in range(3)]
    sigs, pks = eng.sign_batch(msgs, keys), eng.get_public_keys(keys)
    shares = eng.sign_batch([msgs[0]] * 3, keys)
    before = (eng.combine_shares([(ids, shares)]), eng.verify_multiple(sigs, msgs, pks, seed=bytes(32)))
    assert before[0] == ([oracle.sign(msgs[0], b32(coef[0]))[1]], [0]) and before[1][0]
    for g2 in SIDES:
        polys = [[rnd.randrange(1, R) for _ in range(t)] for t in (6, 2, 11)]
        check(eng, sides[g2], polys, [[rnd.getrandbits(256) for _ in range(m)] for m in (40, 70, 9)])
    assert (eng.combine_shares([(ids, shares)]), eng.verify_multiple(sigs, msgs, pks, seed=bytes(32))) == before


# ---- the kernels in use

CHILD = r'''
import importlib, json, os, sys
sys.path.insert(0, %(root)r)
import torch
pkg = importlib.import_module('noble-bls12-381_amd')
eng = pkg.Engine(0)
case = json.loads(sys.stdin.read())
out = {}
for side in ('g1', 'g2'):
    got, st = eng.poly_eval([([bytes.fromhex(c) for c in cs], ids) for cs, ids in case[side]], g2=side == 'g2')
    out[side] = [[b.hex() for b in g] for g in got]
out['kernels'] = [eng.extra_program_kernel(n) for n in ('poly_g1_16', 'poly_g1_256', 'poly_g2_16', 'poly_g2_256')]
out['config'] = eng.config_describe()
print('CHILD_JSON ' + json.dumps(out))
'''


def test_steps_run_on_their_ahead_of_time_kernels_and_the_interpreter_agrees(eng, sides):
    import json
    assert [eng.extra_program_kernel(n) for n in ('poly_g1_16', 'poly_g1_256', 'poly_g2_16', 'poly_g2_256')] == ['nbls_aot_poly_g1', 'nbls_aot_poly_g1', 'nbls_aot_poly_g2', 'nbls_aot_poly_g2']
    with pytest.raises(Exception):
        eng.extra_program_kernel('g1_mul')          # a numbered program is not an extra one
    rnd = random.Random(42)
    case, want = {}, {}
    for g2 in SIDES:
        polys = [[rnd.randrange(1, R) for _ in range(t)] for t in (3, 1, 6)]
        idsets = [[1, 2, 3, 4, 5], [rnd.getrandbits(256), 7], [rnd.getrandbits(256) for _ in range(9)]]
        got, _ = check(eng, sides[g2], polys, idsets)          # the full form (the call holds wide identifiers)
        short, _ = check(eng, sides[g2], polys[:1], idsets[:1])          # and the short one
        assert short[0] == got[0]
        k = 'g2' if g2 else 'g1'
        case[k] = [([c.hex() for c in sides[g2].points(p)], i) for p, i in zip(polys, idsets)]
        want[k] = [[b.hex() for b in g] for g in got]
    e = dict(os.environ); e['NBLS_AOT'] = '0'
    r = subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT}], input=json.dumps(case), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'CHILD_JSON ' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout[r.stdout.index('CHILD_JSON ') + 11:].splitlines()[0])
    assert out['kernels'] == ['nbls_vm_kernel'] * 4 and 'NBLS_AOT=0(env)' in out['config']
    assert out['g1'] == want['g1'] and out['g2'] == want['g2']
