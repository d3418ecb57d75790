"""The scalar field and threshold recombination on the GPU (-m gpu): nbls_fr_op_batch and nbls_lagrange_at_zero against the reference's vectors (ref_fr.json.gz) and Python
integers, nbls_g2_combine_shares / nbls_g1_combine_shares end to end against the oracle.  Keys are Shamir-split in Python integers, the shares are made by the engine's own
sign_batch / get_public_keys (pinned to the reference's vectors by test_gpu_sign.py), combined on the device, and the result has to equal oracle.sign(m, f(0)) and
oracle.get_public_key(f(0)) byte for byte.  Every group of a call is compared with the engine's own sign(m, f(0)); the oracle (5 ms a signature on one core) judges every group
of a call of up to 1100 groups and 514 groups spread over the 8192-group call, its first and last included.  Everything is bit-exact."""
import importlib
import itertools
import random
import pytest
import goldenio
from goldenio import hx

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M256 = (1 << 256) - 1
EDGES = [0, 1, R - 1, R, R + 1, M256]
OPS = ('add', 'sub', 'neg', 'mul', 'sqr', 'inv', 'div', 'pow')
UNARY = ('neg', 'sqr', 'inv')
BAD_IDS = 20
ZERO_SIG = b'\xc0' + bytes(95)
ZERO_PK = b'\xc0' + bytes(47)
SIZES = [1, 63, 64, 65, 4096, 100000]


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


@pytest.fixture(scope='module')
def fr_golden():
    return goldenio.load('ref_fr.json.gz')


def b32(v):
    return v.to_bytes(32, 'big')


def ints(bs):
    return [int.from_bytes(b, 'big') for b in bs]


def py_op(op, a, b):
    a %= R
    if op == 'pow':
        return pow(a, b, R), 0
    b %= R
    if op == 'inv':
        return (0, 5) if a == 0 else (pow(a, -1, R), 0)
    if op == 'div':
        return (0, 5) if b == 0 else (a * pow(b, -1, R) % R, 0)
    return {'add': (a + b) % R, 'sub': (a - b) % R, 'neg': -a % R, 'mul': a * b % R, 'sqr': a * a % R}[op], 0


def py_lagrange(ids):
    x = [v % R for v in ids]
    if 0 in x or len(set(x)) != len(x):
        return None
    out = []
    for k, xk in enumerate(x):
        num = den = 1
        for j, xj in enumerate(x):
            if j != k:
                num = num * xj % R
                den = den * (xj - xk) % R
        out.append(num * pow(den, -1, R) % R)
    return out


# ---- Fr

def test_fr_ops_reference_vectors(eng, fr_golden):
    v = fr_golden['fr_ops']
    a, b, e = ([int(x[k], 16) for x in v] for k in 'abe')
    for op in OPS:
        got, st = eng.fr_op(op, a, None if op in UNARY else (e if op == 'pow' else b))
        for i, x in enumerate(v):
            if x[op] is None:
                assert st[i] == 5 and got[i] == bytes(32), (op, i)
            else:
                assert st[i] == 0 and got[i] == hx(x[op]), (op, i)


@pytest.mark.parametrize('n', SIZES)
def test_fr_ops_python_integers(eng, n):
    rnd = random.Random(n)
    pool = EDGES + [2, R - 2, 2 * R, 2 * R + 1, 1 << 255]
    a = [pool[i % len(pool)] if i % 3 == 0 else rnd.getrandbits(256) for i in range(n)]
    b = [pool[(i // 3) % len(pool)] if i % 5 == 0 else rnd.getrandbits(256) for i in range(n)]
    for op in OPS:
        got, st = eng.fr_op(op, a, None if op in UNARY else b)
        got = ints(got)
        for i in range(n):
            assert (got[i], st[i]) == py_op(op, a[i], b[i]), (op, i, hex(a[i]), hex(b[i]))


# ---- Lagrange coefficients

def check_lagrange(eng, groups, want=None):
    got, st = eng.lagrange_at_zero(groups)
    for g, ids in enumerate(groups):
        w = py_lagrange(ids) if want is None else want[g]
        if w is None:
            assert st[g] == BAD_IDS and got[g] == [bytes(32)] * len(ids), g
        else:
            assert st[g] == 0 and ints(got[g]) == w, (g, len(ids))


def split_sizes(rnd, n):
    """n shares cut into groups of mixed sizes: many of 3, some of 1 .. 130, the rest in one piece when it fits a group"""
    sizes = []
    while n:
        t = min(n, rnd.choice([3, 3, 3, 1, 2, 7, rnd.randrange(1, 131), 667 if n > 5000 and rnd.random() < 0.004 else 5]))
        sizes.append(t)
        n -= t
    return sizes


@pytest.mark.parametrize('n', SIZES)
def test_lagrange_python_integers(eng, n):
    rnd = random.Random(1000 + n)
    if n <= 4096:
        check_lagrange(eng, [list(range(1, n + 1))], want=[binomial_lagrange(n)])          # one group of n
        check_lagrange(eng, [[rnd.getrandbits(256) for _ in range(min(n, 700))]])
    groups = [[rnd.getrandbits(256) if rnd.random() < 0.7 else R + 1 + rnd.randrange(R - 2) for _ in range(t)] for t in split_sizes(rnd, n)]
    check_lagrange(eng, groups)


def binomial_lagrange(t):
    """the coefficients of the identifiers 1 .. t in linear time: lambda_k = prod_{j != k} j / (j - k) = (-1)^(k - 1) C(t, k)"""
    out, c = [], 1
    for k in range(1, t + 1):
        c = c * (t - k + 1) % R * pow(k, -1, R) % R
        out.append(c if k % 2 else -c % R)
    return out


def test_binomial_form_is_the_direct_formula():
    for t in (1, 2, 3, 7, 64, 65):
        assert binomial_lagrange(t) == py_lagrange(list(range(1, t + 1)))


def test_lagrange_one_group_of_65536(eng):
    """identifiers a * pi(j) for a permutation pi of 1 .. t and a random a: lambda_k = prod_{j != k} pi(j) / (pi(j) - pi(k)) = (-1)^(pi(k) - 1) C(t, pi(k)) -- the factor a
    cancels -- which Python computes in linear time where the direct formula is quadratic"""
    t = 65536
    rnd = random.Random(65536)
    a = rnd.getrandbits(255) % R
    pi = list(range(1, t + 1))
    rnd.shuffle(pi)
    by_id = binomial_lagrange(t)
    want = [by_id[p - 1] for p in pi]
    small = [3, 1, 2]
    # beside two small groups, so that the large one starts and ends inside a wavefront
    check_lagrange(eng, [small, [a * p % R for p in pi], small], want=[py_lagrange(small), want, py_lagrange(small)])
    assert want[:3] != [0, 0, 0]


def test_lagrange_bad_identifiers(eng):
    rnd = random.Random(12)
    x = rnd.getrandbits(250)
    good = [rnd.getrandbits(256) for _ in range(70)]
    groups = [good, [1, 2, x, 3, x + R], [4, 5, 6], [7, R, 8], good[:5], [0], [9, 9], [3], good + [good[64]], [1, 2, 3], [2 * R, 5]]
    got, st = eng.lagrange_at_zero(groups)
    assert st == [0, BAD_IDS, 0, BAD_IDS, 0, BAD_IDS, BAD_IDS, 0, BAD_IDS, 0, BAD_IDS]
    check_lagrange(eng, groups)


def test_lagrange_reference_cases(eng, fr_golden):
    cases = fr_golden['threshold']
    check_lagrange(eng, [[int(x, 16) for x in c['ids']] for c in cases], want=[[int(x, 16) for x in c['lambda']] for c in cases])


# ---- recombination

def poly_eval(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % R
    return acc


def make_groups(eng, rnd, sizes, tag, npoly=None, ids_of=None):
    """one polynomial of degree t - 1 per group (npoly: only that many distinct ones, cycled -- Python's side of a call with large groups), identifiers random 256-bit values or
    ids_of(g, t) -> ([(ids, signature shares)], [(ids, key shares)], messages, secrets f(0))"""
    polys = {}
    msgs, secrets, all_ids, keys = [], [], [], []
    for g, t in enumerate(sizes):
        key = (g % npoly, t) if npoly else g
        if key not in polys:
            coef = [rnd.randrange(1, R) for _ in range(t)]
            ids = ids_of(g, t) if ids_of else [rnd.getrandbits(256) for _ in range(t)]
            polys[key] = (coef, ids, [poly_eval(coef, x % R) for x in ids])
        coef, ids, ks = polys[key]
        msgs.append(b'%s group %d' % (tag, g)); secrets.append(coef[0]); all_ids.append(ids); keys.append(ks)
    flat_keys = [b32(k) for ks in keys for k in ks]
    sigs = eng.sign_batch([m for m, ks in zip(msgs, keys) for _ in ks], flat_keys)
    pks = eng.get_public_keys(flat_keys)
    sg, pg, o = [], [], 0
    for ids in all_ids:
        sg.append((ids, sigs[o:o + len(ids)])); pg.append((ids, pks[o:o + len(ids)])); o += len(ids)
    return sg, pg, msgs, secrets


def check_combination(eng, oracle, sg, pg, msgs, secrets, oracle_groups=None):
    sig, st = eng.combine_shares(sg)
    assert st == [0] * len(sg)
    pk, st = eng.combine_shares(pg, g2=False)
    assert st == [0] * len(pg)
    keys = [b32(s) for s in secrets]
    assert sig == eng.sign_batch(msgs, keys)
    assert pk == eng.get_public_keys(keys)
    for g in (range(len(sg)) if oracle_groups is None else oracle_groups):
        assert sig[g] == oracle.sign(msgs[g], keys[g])[1], g
        assert pk[g] == oracle.get_public_key(keys[g]), g
    return sig, pk


@pytest.mark.parametrize('groups,t,npoly', [(1, 1, None), (1, 2, None), (8192, 7, None), (1024, 67, None), (64, 667, 4), (1, 4096, None)])
def test_combine_against_the_oracle(eng, oracle, groups, t, npoly):
    rnd = random.Random(groups * 100003 + t)
    sg, pg, msgs, secrets = make_groups(eng, rnd, [t] * groups, b'%dx%d' % (groups, t), npoly)
    sample = None if groups <= 1100 else sorted(set(range(0, groups, 16)) | {0, groups - 1, groups - 2})
    check_combination(eng, oracle, sg, pg, msgs, secrets, sample)


def test_combine_mixed_group_sizes(eng, oracle):
    rnd = random.Random(130)
    sizes = list(range(1, 131))
    rnd.shuffle(sizes)
    check_combination(eng, oracle, *make_groups(eng, rnd, sizes, b'mixed', ids_of=lambda g, t: list(range(1, t + 1)) if g % 2 else [rnd.getrandbits(256) for _ in range(t)]))


def test_any_subset_gives_the_same_bytes(eng, oracle):
    """n = 9 shares of a degree-3 polynomial: every 4-subset, 5 shares, and all 9 recombine to sign(m, f(0))"""
    rnd = random.Random(9)
    coef = [rnd.randrange(1, R) for _ in range(4)]
    ids = [1, 2, 3, 4, 5, rnd.getrandbits(256), R + 11, 77, 1 << 200]
    keys = [b32(poly_eval(coef, x % R)) for x in ids]
    msg = b'subset'
    sigs, pks = eng.sign_batch([msg] * 9, keys), eng.get_public_keys(keys)
    subsets = [list(c) for c in itertools.combinations(range(9), 4)] + [[8, 1, 6, 3, 0], [4, 3, 2, 1, 0, 5], list(range(9))]
    rnd.shuffle(subsets[0])
    got, st = eng.combine_shares([([ids[i] for i in s], [sigs[i] for i in s]) for s in subsets])
    assert st == [0] * len(subsets) and set(got) == {oracle.sign(msg, b32(coef[0]))[1]}
    got, st = eng.combine_shares([([ids[i] for i in s], [pks[i] for i in s]) for s in subsets], g2=False)
    assert st == [0] * len(subsets) and set(got) == {oracle.get_public_key(b32(coef[0]))}


def test_offsets_need_not_start_at_zero(eng, pkg):
    import ctypes as C
    rnd = random.Random(5)
    sg, pg, msgs, secrets = make_groups(eng, rnd, [2, 3, 4, 1, 5], b'offsets')
    want, _ = eng.combine_shares(sg[2:4])
    ids = b''.join(b32(x) for g in sg for x in g[0])
    shares = b''.join(s for g in sg for s in g[1])
    out, st = C.create_string_buffer(2 * 96), C.create_string_buffer(2)
    assert eng.lib.nbls_g2_combine_shares(eng.h, 2, (C.c_uint32 * 3)(5, 9, 10), ids, shares, out, st) == 0          # groups 2 and 3 of the five, named by absolute offsets
    assert [out.raw[:96], out.raw[96:]] == want and st.raw == bytes(2)
    lam = C.create_string_buffer(5 * 32)
    assert eng.lib.nbls_lagrange_at_zero(eng.h, 2, (C.c_uint32 * 3)(5, 9, 10), ids, lam, None) == 0
    assert ints([lam.raw[32 * k:32 * k + 32] for k in range(5)]) == py_lagrange(sg[2][0]) + py_lagrange(sg[3][0])


def test_status_paths_leave_the_neighbours_alone(eng, oracle, golden):
    rnd = random.Random(20)
    g1, g2 = golden['codec']['g1'], golden['codec']['g2']
    bad = {'g1_sub': [hx(v['hex']) for v in g1 if 'subgroup' in v['result']][0], 'g1_noroot': [hx(v['hex']) for v in g1 if v['result'] == 'Invalid compressed G1 point'][0],
           'g2_sub': [hx(v['hex']) for v in g2 if 'subgroup' in v['result']][0], 'g2_noroot': [hx(v['hex']) for v in g2 if v['result'] == 'Failed to find a square root'][0]}
    sizes = [3, 4, 3, 5, 3, 4, 3, 3, 2, 3, 70, 3]
    sg, pg, msgs, secrets = make_groups(eng, rnd, sizes, b'status', ids_of=lambda g, t: [rnd.randrange(1, 1 << 200) for _ in range(t)])
    good_sig, good_pk = check_combination(eng, oracle, sg, pg, msgs, secrets)
    x = sg[1][0][0]
    want = {1: BAD_IDS, 3: BAD_IDS, 5: BAD_IDS, 6: 3, 7: 4, 8: 1, 10: 4}
    for g2_side, groups, good, zero, e in ((True, sg, good_sig, ZERO_SIG, 96), (False, pg, good_pk, ZERO_PK, 48)):
        gs = [(list(i), list(s)) for i, s in groups]
        gs[1][0][2] = x                                                   # duplicate identifiers
        gs[3][0][4] = 0                                                   # a zero identifier
        gs[5][0][3] = gs[5][0][1] + R                                     # the x / x + r collision
        gs[6][1][1] = bad['g2_sub' if g2_side else 'g1_sub']              # a share outside the subgroup
        gs[7][1][2] = bad['g2_noroot' if g2_side else 'g1_noroot']        # a share with no square root
        gs[10][1][66] = bad['g2_noroot' if g2_side else 'g1_noroot']      # ... behind a tile boundary, and a subgroup failure after it: the first one is reported
        gs[10][1][69] = bad['g2_sub' if g2_side else 'g1_sub']
        # group 8: shares s and [2]s with identifiers 1 and 2: lambda = (2, -1), 2s - 2s is the zero point
        h = oracle.hash_to_g2(b'zero combination')[1] if g2_side else oracle.g1_generator()
        mul = oracle.g2_mul if g2_side else oracle.g1_mul
        comp = eng.compress_batch(mul(h, 5)[1] + mul(h, 10)[1], g2=g2_side)
        gs[8] = ([1, 2], [comp[:e], comp[e:]])
        # group 9: a zero share is valid and adds nothing -- what remains is lambda_0 s_0 + lambda_2 s_2
        gs[9][1][1] = zero
        got, st = eng.combine_shares(gs, g2=g2_side)
        for g in range(len(gs)):
            if g == 9:
                continue
            assert st[g] == want.get(g, 0), (g2_side, g)
            assert got[g] == (zero if st[g] == 1 else bytes(e) if st[g] else good[g]), (g2_side, g)
        lam = py_lagrange(gs[9][0])
        aff, dst = eng.decompress_batch(gs[9][1][0] + gs[9][1][2], g2=g2_side)
        a = 2 * e
        parts = mul(aff[:a], lam[0])[1] + mul(aff[a:], lam[2])[1]
        total = (oracle.g2_sum if g2_side else oracle.g1_sum)(parts)[1]
        assert st[9] == 0 and dst == [0, 0] and got[9] == eng.compress_batch(total, g2=g2_side)
    # a group that is nothing but zero shares combines to the zero point
    got, st = eng.combine_shares([([1, 2, 3], [ZERO_SIG] * 3), sg[0]])
    assert st == [1, 0] and got == [ZERO_SIG, good_sig[0]]


def test_reference_made_cases(eng, fr_golden):
    cases = fr_golden['threshold']
    ids = [[int(x, 16) for x in c['ids']] for c in cases]
    got, st = eng.combine_shares([(i, [hx(s) for s in c['sig_shares']]) for i, c in zip(ids, cases)])
    assert st == [0] * len(cases) and got == [hx(c['sig']) for c in cases]
    got, st = eng.combine_shares([(i, [hx(s) for s in c['pk_shares']]) for i, c in zip(ids, cases)], g2=False)
    assert st == [0] * len(cases) and got == [hx(c['pk']) for c in cases]
    # identifiers as 32-byte values
    got, st = eng.combine_shares([([hx(x) for x in c['ids']], [hx(s) for s in c['sig_shares']]) for c in cases])
    assert got == [hx(c['sig']) for c in cases]


def test_verify_shares_combine_verify_and_other_calls_still_match(eng, oracle):
    """the use the calls are for -- verify the shares, combine them, verify the result under the group key -- and then verifyBatch and a pairing on the same context against
    the oracle: the new scratch slots collide with nothing"""
    rnd = random.Random(77)
    sg, pg, msgs, secrets = make_groups(eng, rnd, [5, 3, 9], b'flow')
    for (ids, sigs), (_, pks), m in zip(sg, pg, msgs):
        ok, st = eng.verify_multiple(sigs, [m] * len(sigs), pks)
        assert ok and not any(st)
    sig, _ = eng.combine_shares(sg)
    pk, _ = eng.combine_shares(pg, g2=False)
    ok, st = eng.verify_multiple(sig, msgs, pk)
    assert ok and not any(st)
    for s, m, p in zip(sig, msgs, pk):
        assert oracle.verify(s, m, p) == 1
    # verifyBatch of the three group signatures' aggregate, and a pairing
    agg = oracle.aggregate_signatures(sig)
    agg = agg[1] if isinstance(agg, tuple) else agg
    assert eng.verify_batch(agg, msgs, pk) is True
    assert oracle.verify_batch(agg, msgs, pk) == 1
    G1 = b''.join(oracle.g1_mul(oracle.g1_generator(), k)[1] for k in (3, 11))
    G2 = b''.join(oracle.g2_mul(oracle.g2_generator(), k)[1] for k in (5, 13))
    assert eng.pairing_batch(G1, G2, True, False)[0] == oracle.pairing_batch(G1, G2, True, False)[0]
    # and the combination again, after them
    assert eng.combine_shares(sg)[0] == sig
