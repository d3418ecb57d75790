"""nbls_verify_aggregates / nbls_verify_aggregates_indexed on the GPU (-m gpu): n sets (signature, message, keys) checked together by a random linear combination over the sets,
every status against what the oracle does for verify(sig_j, m_j, aggregatePublicKeys(keys_j)) -- the aggregate's decoder status when a key does not decode, else verify's
answer mapped as nbls_verify_multiple's statuses are (test_gpu_verify_multiple.py expected)."""
import hashlib
import importlib
import random
import pytest
from goldenio import hx

pytestmark = pytest.mark.gpu
DST = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ZERO_PK = b'\xc0' + bytes(47)
ZERO_SIG = b'\xc0' + bytes(95)
SEEDS = [hashlib.sha256(b'aggregate seed %d' % k).digest() for k in range(3)]
EINVAL = -1


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


@pytest.fixture(scope='module')
def bad_keys(golden):
    g1 = golden['codec']['g1']
    sub = [hx(v['hex']) for v in g1 if 'subgroup' in v['result']]
    noroot = [hx(v['hex']) for v in g1 if v['result'] == 'Invalid compressed G1 point']
    g2 = golden['codec']['g2']
    return sub, noroot, [hx(v['hex']) for v in g2 if 'subgroup' in v['result']], [hx(v['hex']) for v in g2 if v['result'] == 'Failed to find a square root']


def expected(oracle, sig, msg, keys, dst=DST):
    """oracle: aggregatePublicKeys(keys), then verify(sig, msg, aggregate) -> the status nbls_verify_aggregates reports for the set"""
    st, agg = oracle.aggregate_public_keys(keys)
    if st < 0:
        return -st
    v = oracle.verify(sig, msg, agg, dst)
    if v == 1:
        return 0
    if v == 0:
        return 9
    if v == -1:
        return 1 if agg == ZERO_PK else 11
    return -v


def neg(pk):
    """-P of a compressed non-zero G1 point: the sort flag (bit 5 of the first byte) flipped"""
    return bytes([pk[0] ^ 0x20]) + pk[1:]


def make_sets(eng, rnd, sizes, tag=b''):
    """valid sets: set j has sizes[j] fresh keys and the aggregate signature sign(m_j, sum sk mod r) -> (sigs, msgs, key_sets, secret keys per set)"""
    sks = [[rnd.randrange(1, R) for _ in range(k)] for k in sizes]
    flat = [k.to_bytes(32, 'big') for s in sks for k in s]
    pks = eng.get_public_keys(flat)
    key_sets, at = [], 0
    for k in sizes:
        key_sets.append(pks[at:at + k])
        at += k
    msgs = [tag + b'aggregate %d ' % j + rnd.getrandbits(64).to_bytes(8, 'big') for j in range(len(sizes))]
    agg = [(sum(s) % R).to_bytes(32, 'big') for s in sks]
    return eng.sign_batch(msgs, agg), msgs, key_sets, sks


def check(eng, oracle, sigs, msgs, key_sets, seed=SEEDS[0]):
    exp = [expected(oracle, s, m, k) for s, m, k in zip(sigs, msgs, key_sets)]
    ok, st = eng.verify_aggregates(sigs, msgs, key_sets, seed=seed)
    assert list(st) == exp
    assert ok == all(e == 0 for e in exp)
    ok2, st2 = eng.verify_aggregates(sigs, msgs, key_sets, seed=seed, per_set=False)
    assert st2 is None and ok2 == ok
    return list(st)


@pytest.mark.parametrize('k', [1, 2, 3, 63, 64, 65, 512])
def test_valid_sets(eng, oracle, k):
    rnd = random.Random(1000 + k)
    n = 6 if k < 512 else 3
    sizes = [k] * n
    sigs, msgs, key_sets, _ = make_sets(eng, rnd, sizes)
    for j in (0, n - 1):
        assert expected(oracle, sigs[j], msgs[j], key_sets[j]) == 0
    for seed in (SEEDS[1], None):
        ok, st = eng.verify_aggregates(sigs, msgs, key_sets, seed=seed)
        assert ok and st == bytes(n)
        ok, st = eng.verify_aggregates(sigs, msgs, key_sets, seed=seed, per_set=False)
        assert ok and st is None
    # mixed sizes in one call, the largest set last and first
    sizes = [k, 1, 2, 7, k + 1]
    sigs, msgs, key_sets, _ = make_sets(eng, rnd, sizes, b'mixed')
    ok, st = eng.verify_aggregates(sigs, msgs, key_sets, seed=SEEDS[1])
    assert ok and st == bytes(len(sizes))


def test_malformed_sets(eng, oracle, bad_keys):
    g1_sub, g1_noroot, g2_sub, g2_noroot = bad_keys
    rnd = random.Random(77)
    sizes = [5] * 18
    sigs, msgs, key_sets, sks = make_sets(eng, rnd, sizes, b'malformed')
    ks = [list(k) for k in key_sets]
    ks[0][0] = g1_sub[0]                                     # outside the subgroup: first, in the middle, last
    ks[1][2] = g1_sub[0]
    ks[2][4] = g1_sub[-1]
    ks[3][1], ks[3][3] = g1_noroot[0], g1_sub[0]            # two bad keys: the first one's status
    ks[4][1], ks[4][3] = g1_sub[0], g1_noroot[0]
    ks[5][2] = g1_noroot[-1]                                 # no square root
    ks[6].insert(3, ZERO_PK)                                 # a zero key among valid keys adds nothing
    ks[7] = [ks[7][0], neg(ks[7][0])]                        # {pk, -pk}: the aggregate is the zero point
    ks[8] = [ZERO_PK, ZERO_PK]                               # only zero keys
    ks[9] = [ks[9][0], ks[9][0], ks[9][1]]                   # the same key twice: a doubling inside the complete addition
    sigs[9] = eng.sign_batch([msgs[9]], [((2 * sks[9][0] + sks[9][1]) % R).to_bytes(32, 'big')])[0]
    sigs[10] = g2_sub[0]                                     # a bad signature
    sigs[11] = g2_noroot[0] if g2_noroot else g2_sub[-1]
    sigs[12] = ZERO_SIG                                      # a zero signature
    msgs[13] = msgs[13] + b'!'                               # a wrong message
    sigs[14] = eng.sign_batch([msgs[14]], [(sum(sks[14][:3]) % R).to_bytes(32, 'big')])[0]   # signed by a subset of the keys
    ks[15], ks[16] = ks[16], ks[15]                          # key lists swapped between two sets
    ks[17][0], sigs[17] = g1_sub[0], g2_sub[0]               # a bad key AND a bad signature: the key's status, as in the reference
    st = check(eng, oracle, sigs, msgs, ks)
    assert st[:10] == [3, 3, 3, 4, 3, 4, 0, 1, 1, 0]
    assert st[10] == 13 and st[11] in (13, 14) and st[12] == 11
    assert st[13:] == [9, 9, 9, 9, 3]
    for seed in SEEDS[1:]:
        ok, st2 = eng.verify_aggregates(sigs, msgs, ks, seed=seed)
        assert not ok and list(st2) == st


def test_cancellation_across_sets(eng, oracle):
    """sig_a + D and sig_b - D: the plain sum of the signatures is unchanged, the weighted one is not"""
    rnd = random.Random(91)
    sigs, msgs, key_sets, _ = make_sets(eng, rnd, [4, 9, 1, 16, 3, 8], b'cancel')
    g2 = oracle.g2_generator()
    d = 0x1234567890abcdef1234567890abcdef
    D, negD = oracle.g2_mul(g2, d)[1], oracle.g2_mul(g2, R - d)[1]
    aff, st = oracle.decompress_batch(b''.join(sigs), g2=True)
    assert st == bytes(6)
    a1 = oracle.g2_sum(aff[1 * 192:2 * 192] + D)[1]
    a4 = oracle.g2_sum(aff[4 * 192:5 * 192] + negD)[1]
    comp = eng.compress_batch(a1 + a4, g2=True)
    bad = list(sigs)
    bad[1], bad[4] = comp[:96], comp[96:]
    aff2, _ = oracle.decompress_batch(b''.join(bad), g2=True)
    assert oracle.g2_sum(aff2)[1] == oracle.g2_sum(aff)[1]
    for seed in SEEDS:
        ok, st = eng.verify_aggregates(bad, msgs, key_sets, seed=seed)
        assert not ok and list(st) == [0, 9, 0, 0, 9, 0]
        ok, st = eng.verify_aggregates(bad, msgs, key_sets, seed=seed, per_set=False)
        assert not ok and st is None


def test_singletons_match_verify_multiple(eng, oracle):
    n = 65536
    rnd = random.Random(65536)
    sks = [rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(n)]
    msgs = [rnd.getrandbits(64).to_bytes(8, 'big') for _ in range(n)]
    sigs, pks = eng.sign_batch(msgs, sks), eng.get_public_keys(sks)
    key_sets = [[p] for p in pks]
    for seed in (SEEDS[0], SEEDS[2]):
        assert eng.verify_aggregates(sigs, msgs, key_sets, seed=seed) == eng.verify_multiple(sigs, msgs, pks, seed=seed) == (True, bytes(n))
    msgs[7], sigs[n - 1] = msgs[7] + b'x', sigs[0]
    for j in (7, n - 1):
        assert expected(oracle, sigs[j], msgs[j], key_sets[j]) == 9
    want = eng.verify_multiple(sigs, msgs, pks, seed=SEEDS[0])
    assert want[0] is False and [i for i, v in enumerate(want[1]) if v] == [7, n - 1]
    assert eng.verify_aggregates(sigs, msgs, key_sets, seed=SEEDS[0]) == want
    assert eng.verify_aggregates(sigs, msgs, key_sets, seed=SEEDS[0], per_set=False) == (False, None)


def test_keyset_statuses(eng, oracle, bad_keys):
    g1_sub, g1_noroot = bad_keys[0], bad_keys[1]
    rnd = random.Random(5)
    pks = eng.get_public_keys([rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(200)])
    pks[3], pks[50], pks[51], pks[199] = ZERO_PK, g1_sub[0], g1_noroot[0], g1_sub[-1]
    ks, st = eng.create_keyset(pks)
    try:
        assert len(ks) == 200
        assert st == oracle.decompress_batch(b''.join(pks))[1]
        assert [i for i, v in enumerate(st) if v] == [3, 50, 51, 199]
    finally:
        ks.close()
    assert ks.h is None


@pytest.fixture(scope='module')
def big_table(eng):
    """8192 keys in a table, 256 sets of 512 indices each (keys shared between sets), valid aggregate signatures"""
    rnd = random.Random(256)
    sk = [rnd.randrange(1, R) for _ in range(8192)]
    pks = eng.get_public_keys([k.to_bytes(32, 'big') for k in sk])
    ks, st = eng.create_keyset(pks)
    assert st == bytes(8192)
    idx = [[rnd.randrange(8192) for _ in range(512)] for _ in range(256)]
    msgs = [b'table set %d' % j for j in range(256)]
    sigs = eng.sign_batch(msgs, [(sum(sk[i] for i in s) % R).to_bytes(32, 'big') for s in idx])
    yield ks, pks, sk, idx, msgs, sigs
    ks.close()


def test_indexed_equals_per_call(eng, oracle, big_table):
    ks, pks, sk, idx, msgs, sigs = big_table
    key_sets = [[pks[i] for i in s] for s in idx]
    for j in (0, 255):
        assert expected(oracle, sigs[j], msgs[j], key_sets[j]) == 0
    want = eng.verify_aggregates(sigs, msgs, key_sets, seed=SEEDS[0])
    assert want == (True, bytes(256))
    assert eng.verify_aggregates_indexed(ks, sigs, msgs, idx, seed=SEEDS[0]) == want
    assert eng.verify_aggregates_indexed(ks, sigs, msgs, idx, seed=SEEDS[0], per_set=False) == (True, None)
    bad = list(msgs)
    bad[17] = b'not signed'
    sigs2 = list(sigs)
    sigs2[200] = sigs[201]
    want = eng.verify_aggregates(sigs2, bad, key_sets, seed=SEEDS[1])
    assert want[0] is False and [i for i, v in enumerate(want[1]) if v] == [17, 200] and set(want[1]) == {0, 9}
    assert eng.verify_aggregates_indexed(ks, sigs2, bad, idx, seed=SEEDS[1]) == want
    assert eng.verify_aggregates_indexed(ks, sigs2, bad, idx, seed=SEEDS[1], per_set=False) == (False, None)


def test_indexed_shared_and_bad_keys(eng, oracle, bad_keys):
    g1_sub = bad_keys[0]
    rnd = random.Random(12)
    sk = [rnd.randrange(1, R) for _ in range(6)]
    pks = eng.get_public_keys([k.to_bytes(32, 'big') for k in sk]) + [ZERO_PK, g1_sub[0]]
    ks, st = eng.create_keyset(pks)
    try:
        assert list(st) == [0] * 6 + [1, 3]
        idx = [[0, 1, 2], [1, 2, 3], [0, 3], [4], [4, 6, 5], [5, 5], [2, 7, 1], [6], [0, 0, 0, 1]]
        msgs = [b'shared %d' % j for j in range(len(idx))]
        sigs = eng.sign_batch(msgs, [(sum(sk[i] for i in s if i < 6) % R or 1).to_bytes(32, 'big') for s in idx])
        key_sets = [[pks[i] for i in s] for s in idx]
        exp = [expected(oracle, s, m, k) for s, m, k in zip(sigs, msgs, key_sets)]
        assert exp == [0, 0, 0, 0, 0, 0, 3, 1, 0]
        for seed in SEEDS:
            assert eng.verify_aggregates_indexed(ks, sigs, msgs, idx, seed=seed) == (False, bytes(exp))
            assert eng.verify_aggregates(sigs, msgs, key_sets, seed=seed) == (False, bytes(exp))
        # an index out of range: refused, nothing run
        with pytest.raises(Exception, match=r'code %d\b' % EINVAL):
            eng.verify_aggregates_indexed(ks, sigs, msgs, idx[:-1] + [[0, 8]], seed=SEEDS[0])
    finally:
        ks.close()


def test_second_context_uses_table(pkg, eng, big_table):
    ks, pks, sk, idx, msgs, sigs = big_table
    other = pkg.Engine(0)
    try:
        want = eng.verify_aggregates_indexed(ks, sigs[:64], msgs[:64], idx[:64], seed=SEEDS[2])
        assert want == (True, bytes(64))
        assert other.verify_aggregates_indexed(ks, sigs[:64], msgs[:64], idx[:64], seed=SEEDS[2]) == want
        swapped = list(idx[:64])
        swapped[5], swapped[6] = swapped[6], swapped[5]
        assert other.verify_aggregates_indexed(ks, sigs[:64], msgs[:64], swapped, seed=SEEDS[2]) == (False, bytes(5) + b'\x09\x09' + bytes(57))
    finally:
        other.close()


def test_refused_calls(eng):
    lib, h = eng.lib, eng.h
    import ctypes as C
    ok = C.c_int(0)
    sig, pk, msg = ZERO_SIG, ZERO_PK, b'm'
    off = (C.c_uint32 * 2)(0, 1)
    empty = (C.c_uint32 * 3)(0, 1, 1)
    two = (C.c_uint32 * 3)(0, 1, 2)
    down = (C.c_uint32 * 3)(0, 2, 1)
    assert lib.nbls_verify_aggregates(h, 2, sig * 2, msg * 2, two, pk * 2, empty, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert lib.nbls_verify_aggregates(h, 2, sig * 2, msg * 2, two, pk * 2, down, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert lib.nbls_verify_aggregates(h, 0, sig, msg, off, pk, off, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert lib.nbls_verify_aggregates(h, 1, sig, msg, off, None, off, DST, len(DST), None, C.byref(ok), None) == EINVAL
    big = (C.c_uint32 * 2)(0, (1 << 24) + 1)
    assert lib.nbls_verify_aggregates(h, 1, sig, msg, off, pk, big, DST, len(DST), None, C.byref(ok), None) == EINVAL


def test_scratch_intact_after(eng, oracle, golden):
    rnd = random.Random(3)
    sigs, msgs, key_sets, _ = make_sets(eng, rnd, [40, 2, 7], b'scratch')
    sigs[1] = sigs[2]
    ok, st = eng.verify_aggregates(sigs, msgs, key_sets, seed=SEEDS[0])
    assert not ok and list(st) == [0, 9, 0]
    ms = [b'scratch %d' % i for i in range(8)]
    apk, agg = oracle.aggregate_sign(ms, [bytes([7 + i]) * 32 for i in range(8)])
    assert oracle.verify_batch(agg, ms, apk) == 1
    assert eng.verify_batch(agg, ms, apk) is True
    assert eng.verify_batch(agg, ms[::-1], apk) is False
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:6])
    g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:6])
    out, _ = eng.pairing_batch(g1, g2, True, False)
    assert out == oracle.pairing_batch(g1, g2, True, False)[0]
