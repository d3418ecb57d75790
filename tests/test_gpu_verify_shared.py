"""The shared-message entry points on the GPU (-m gpu): n sets over m <= n messages, one hash-to-G2 and one Miller loop per MESSAGE.  Every case is checked twice: against the
oracle's verify(sig_i, msgs[msg_index[i]], pk_i) per set (the mapping of test_gpu_verify_multiple.py expected / test_gpu_verify_aggregates.py expected), and against the existing
entry point on the expanded input with the same seed, which the shared call must equal byte for byte (statuses and all_ok).  The oracle judges every set of a case of up to 65
sets and every set a case alters; above that a sample of 24 sets plus the altered ones."""
import ctypes as C
import hashlib
import importlib
import math
import random
import pytest
from goldenio import hx

pytestmark = pytest.mark.gpu
DST = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ZERO_PK = b'\xc0' + bytes(47)
ZERO_SIG = b'\xc0' + bytes(95)
SEEDS = [hashlib.sha256(b'shared seed %d' % k).digest() for k in range(3)]
EINVAL = -1


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def expected(v, pk):
    """oracle.verify's answer -> the status nbls_verify_multiple reports for the set (test_gpu_verify_multiple.py expected)"""
    if v == 1:
        return 0
    if v == 0:
        return 9
    if v == -1:
        return 1 if pk == ZERO_PK else 11
    return -v


def agg_expected(oracle, sig, msg, keys):
    """oracle: aggregatePublicKeys(keys), then verify -> the status nbls_verify_aggregates reports (test_gpu_verify_aggregates.py expected)"""
    st, agg = oracle.aggregate_public_keys(keys)
    if st < 0:
        return -st
    return expected(oracle.verify(sig, msg, agg, DST), agg)


def random_index(rnd, n, m):
    """a random map of n sets ONTO m messages, groups not contiguous"""
    idx = list(range(m)) + [rnd.randrange(m) for _ in range(n - m)]
    rnd.shuffle(idx)
    return idx


def shared_sets(eng, rnd, n, m, index=None, tag=b''):
    """n valid sets over m distinct messages -> (sigs, distinct messages, index, keys, secret keys)"""
    index = random_index(rnd, n, m) if index is None else index
    sks = [rnd.randrange(1, R) for _ in range(n)]
    msgs = [tag + b'root %d ' % g + rnd.getrandbits(64).to_bytes(8, 'big') * (1 + g % 3) for g in range(m)]
    raw = [k.to_bytes(32, 'big') for k in sks]
    return eng.sign_batch([msgs[g] for g in index], raw), msgs, index, eng.get_public_keys(raw), sks


def judged(rnd, n, altered=()):
    return list(range(n)) if n <= 65 else sorted(set(rnd.sample(range(n), 24)) | set(altered))


def check(eng, oracle, sigs, msgs, index, pks, seed=SEEDS[0], altered=(), fast_equal=True):
    """the shared call == the existing call on the expanded input == the oracle (on the judged sets); per_set=False gives the same all_ok -> statuses as a list"""
    n = len(sigs)
    full = [msgs[g] for g in index]
    ok, st = eng.verify_multiple_shared(sigs, msgs, index, pks, seed=seed)
    assert (ok, st) == eng.verify_multiple(sigs, full, pks, seed=seed)
    for i in judged(random.Random(n), n, altered):
        assert st[i] == expected(oracle.verify(sigs[i], full[i], pks[i], DST), pks[i]), i
    assert ok == (st == bytes(n))
    if fast_equal:
        assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=seed, per_set=False) == (ok, None)
    return list(st)


def ms_for(n):
    return sorted({1, min(2, n), max(1, math.isqrt(n)), n})


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 1000, 4097])
def test_valid_sets(eng, oracle, n):
    rnd = random.Random(7000 + n)
    for m in ms_for(n):
        sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, m)
        assert check(eng, oracle, sigs, msgs, index, pks, SEEDS[1]) == [0] * n, m
    # the identity index; and the seed from the OS
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, n, list(range(n)))
    assert check(eng, oracle, sigs, msgs, index, pks, SEEDS[2]) == [0] * n
    assert eng.verify_multiple_shared(sigs, msgs, index, pks) == (True, bytes(n))
    # one group of n, then its last set altered
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, 1)
    assert index == [0] * n
    assert check(eng, oracle, sigs, msgs, index, pks, SEEDS[0]) == [0] * n
    sigs[-1] = eng.sign_batch([b'something else'], [bytes(31) + b'\x05'])[0]
    assert check(eng, oracle, sigs, msgs, index, pks, SEEDS[0], altered=[n - 1]) == [0] * (n - 1) + [9]


def test_repeated_messages_in_msgs(eng, oracle):
    """the caller need not dedupe perfectly: the same bytes at two places of msgs"""
    rnd = random.Random(11)
    sigs, msgs, index, pks, sks = shared_sets(eng, rnd, 40, 5)
    msgs[3] = msgs[1]
    sigs = eng.sign_batch([msgs[g] for g in index], [k.to_bytes(32, 'big') for k in sks])
    assert check(eng, oracle, sigs, msgs, index, pks) == [0] * 40


def test_reference_sign_vectors(pkg, eng, oracle, testdata):
    vs = testdata['sign_vectors']
    sigs, flat, pks = [hx(v[2]) for v in vs], [hx(v[1]) for v in vs], eng.get_public_keys([hx(v[0]) for v in vs])
    msgs, index = pkg.group_messages(flat)
    assert len(flat) == 559 and len(msgs) == 532 and [msgs[g] for g in index] == flat
    assert check(eng, oracle, sigs, msgs, index, pks) == [0] * 559
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=None, per_set=False) == (True, None)


def test_swap_attack(eng, oracle):
    """two signers of one message with their signatures exchanged: sig_a + sig_b is unchanged, so an unweighted same-message sum would accept; the weights are per set"""
    rnd = random.Random(21)
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, 30, 4)
    a, b = [i for i, g in enumerate(index) if g == index[0]][:2]
    sigs[a], sigs[b] = sigs[b], sigs[a]
    for seed in SEEDS:
        st = check(eng, oracle, sigs, msgs, index, pks, seed)
        assert st == [9 if i in (a, b) else 0 for i in range(30)]


def test_cancellation_inside_one_group(eng, oracle):
    """sig_a + D and sig_b - D for two signers of one message"""
    rnd = random.Random(22)
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, 24, 3)
    a, b = [i for i, g in enumerate(index) if g == 1][:2]
    g2 = oracle.g2_generator()
    d = 0x1234567890abcdef1234567890abcdef
    D, negD = oracle.g2_mul(g2, d)[1], oracle.g2_mul(g2, R - d)[1]
    aff, st = oracle.decompress_batch(b''.join(sigs), g2=True)
    assert st == bytes(24)
    pa = oracle.g2_sum(aff[a * 192:(a + 1) * 192] + D)[1]
    pb = oracle.g2_sum(aff[b * 192:(b + 1) * 192] + negD)[1]
    comp = eng.compress_batch(pa + pb, g2=True)
    bad = list(sigs)
    bad[a], bad[b] = comp[:96], comp[96:]
    aff2, _ = oracle.decompress_batch(b''.join(bad), g2=True)
    assert oracle.g2_sum(aff2)[1] == oracle.g2_sum(aff)[1]
    for seed in SEEDS:
        assert check(eng, oracle, bad, msgs, index, pks, seed) == [9 if i in (a, b) else 0 for i in range(24)]


def test_wrong_message_index(eng, oracle):
    rnd = random.Random(23)
    # (8, 3): the per-set pass gathers H(m) through an unordered index; its 8 x 36 vectors cross the first workgroup inside a set, and every status meets the oracle's
    for n, m, index in ((20, 4, None), (300, 17, None), (8, 3, [2, 0, 1, 0, 2, 1, 0, 2])):
        sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, m, index)
        k = next(i for i, g in enumerate(index) if index.count(g) >= 2)      # its message keeps another signer: the map stays onto 0 .. m - 1
        index[k] = (index[k] + 1) % m
        assert check(eng, oracle, sigs, msgs, index, pks, altered=[k]) == [9 if i == k else 0 for i in range(n)]


def test_malformed_inside_large_groups(eng, oracle, golden):
    g1 = golden['codec']['g1']
    g1_sub = [hx(v['hex']) for v in g1 if 'subgroup' in v['result']][0]
    g1_noroot = [hx(v['hex']) for v in g1 if v['result'] == 'Invalid compressed G1 point'][0]
    g2_sub = [hx(v['hex']) for v in golden['codec']['g2'] if 'subgroup' in v['result']][0]
    rnd = random.Random(24)
    n = 200
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, 3)
    pks[0] = ZERO_PK                                          # 1
    pks[20] = g1_sub                                          # 3
    pks[41] = g1_noroot                                       # 4
    sigs[77] = ZERO_SIG                                       # 11
    sigs[100] = g2_sub                                        # 13
    pks[150], sigs[150] = ZERO_PK, g2_sub                     # the signature's code wins, as in the reference
    want = {0: 1, 20: 3, 41: 4, 77: 11, 100: 13, 150: 13}
    full = [msgs[g] for g in index]
    exp = [expected(oracle.verify(s, m_, p, DST), p) for s, m_, p in zip(sigs, full, pks)]      # every set: the group mates are judged too
    assert exp == [want.get(i, 0) for i in range(n)]
    for seed in SEEDS[:2]:
        assert check(eng, oracle, sigs, msgs, index, pks, seed, altered=list(want)) == exp


def weight(seed, i):
    """the header's formula: r_i = BE64(SHA-256(seed || BE64(i))[0..8]) | 2^63"""
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, 'big')).digest()[:8], 'big') | 1 << 63


@pytest.mark.parametrize('others', [60, 300])
def test_zero_group_sum(eng, oracle, others):
    """[r_a]pk_a + [r_b]pk_b = 0 for the two signers of one message: that group's key cannot go into a Miller loop.  The sets are valid, so with statuses every one is 0; the
    combined check alone cannot count and answers false -- the documented price -- and nothing faults"""
    seed = SEEDS[1]
    rnd = random.Random(25 + others)
    n = others + 2
    a, b = 5, others // 2
    m = 6
    index = random_index(rnd, others, m - 1)
    index.insert(a, m - 1)
    index.insert(b, m - 1)
    assert [i for i, g in enumerate(index) if g == m - 1] == [a, b]
    sigs, msgs, index, pks, sks = shared_sets(eng, rnd, n, m, index)
    sks[b] = (-sks[a] * weight(seed, a) * pow(weight(seed, b), -1, R)) % R
    assert (sks[a] * weight(seed, a) + sks[b] * weight(seed, b)) % R == 0
    raw = sks[b].to_bytes(32, 'big')
    pks[b], sigs[b] = eng.get_public_keys([raw])[0], eng.sign_batch([msgs[m - 1]], [raw])[0]
    assert oracle.verify(sigs[b], msgs[m - 1], pks[b], DST) == 1
    st = check(eng, oracle, sigs, msgs, index, pks, seed, altered=[a, b], fast_equal=False)
    assert st == [0] * n
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=seed) == (True, bytes(n))
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=seed, per_set=False) == (False, None)
    # another seed: the sum is not zero, the combined check counts
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=SEEDS[2], per_set=False) == (True, None)
    # and an invalid set elsewhere is still found
    sigs[0] = sigs[1]
    assert check(eng, oracle, sigs, msgs, index, pks, seed, altered=[0, a, b], fast_equal=False) == [9] + [0] * (n - 1)


def test_three_forms_agree(pkg, eng, oracle):
    rnd = random.Random(26)
    n, m = 500, 22
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, m)
    sigs[3], sigs[400] = sigs[400], sigs[3]
    want = eng.verify_multiple_shared(sigs, msgs, index, pks, seed=SEEDS[0])
    full = [msgs[g] for g in index]
    assert want[0] is False and want == eng.verify_multiple(sigs, full, pks, seed=SEEDS[0])
    for i in (3, 400, 0, n - 1):
        assert want[1][i] == expected(oracle.verify(sigs[i], full[i], pks[i], DST), pks[i])
    singles = [[p] for p in pks]
    assert eng.verify_aggregates_shared(sigs, msgs, index, singles, seed=SEEDS[0]) == want
    assert eng.verify_aggregates_shared(sigs, msgs, index, singles, seed=SEEDS[0], per_set=False) == (False, None)
    ks, st = eng.create_keyset(pks)
    other = pkg.Engine(0)
    try:
        assert st == bytes(n)
        idx = [[i] for i in range(n)]
        assert eng.verify_aggregates_indexed_shared(ks, sigs, msgs, index, idx, seed=SEEDS[0]) == want
        assert other.verify_aggregates_indexed_shared(ks, sigs, msgs, index, idx, seed=SEEDS[0]) == want
    finally:
        other.close()
        ks.close()


def test_aggregate_sets_share_messages(pkg, eng, oracle):
    """sets of several keys each over a few messages: per-call and indexed forms, against their twins on the expanded input and the oracle"""
    rnd = random.Random(27)
    nkeys, n, m = 96, 40, 5
    sk = [rnd.randrange(1, R) for _ in range(nkeys)]
    pks = eng.get_public_keys([k.to_bytes(32, 'big') for k in sk])
    idx = [[rnd.randrange(nkeys) for _ in range(1 + (7 * j) % 13)] for j in range(n)]
    index = random_index(rnd, n, m)
    msgs = [b'attestation root %d' % g for g in range(m)]
    full = [msgs[g] for g in index]
    sigs = eng.sign_batch(full, [(sum(sk[i] for i in s) % R).to_bytes(32, 'big') for s in idx])
    key_sets = [[pks[i] for i in s] for s in idx]
    sigs[9], sigs[30] = sigs[30], sigs[9]
    key_sets[17] = key_sets[17] + [ZERO_PK]              # adds nothing
    key_sets[21] = [ZERO_PK]                              # the aggregate is the zero point: 1
    exp = bytes(agg_expected(oracle, s, m_, k) for s, m_, k in zip(sigs, full, key_sets))
    assert [i for i, v in enumerate(exp) if v] == sorted({9, 30, 21}) and exp[21] == 1
    ks, st = eng.create_keyset(pks + [ZERO_PK])
    other = pkg.Engine(0)
    try:
        idx2 = [list(s) for s in idx]
        idx2[17] = idx2[17] + [nkeys]
        idx2[21] = [nkeys]
        for seed in SEEDS[:2]:
            want = eng.verify_aggregates(sigs, full, key_sets, seed=seed)
            assert want == (False, exp)
            assert eng.verify_aggregates_shared(sigs, msgs, index, key_sets, seed=seed) == want
            assert eng.verify_aggregates_indexed(ks, sigs, full, idx2, seed=seed) == want
            assert eng.verify_aggregates_indexed_shared(ks, sigs, msgs, index, idx2, seed=seed) == want
            assert other.verify_aggregates_indexed_shared(ks, sigs, msgs, index, idx2, seed=seed) == want
            assert eng.verify_aggregates_shared(sigs, msgs, index, key_sets, seed=seed, per_set=False) == (False, None)
        # all valid
        sigs[9], sigs[30] = sigs[30], sigs[9]
        key_sets[21], idx2[21] = [pks[i] for i in idx[21]], idx[21]
        for j in (0, 9, 21, 30, n - 1):
            assert agg_expected(oracle, sigs[j], full[j], key_sets[j]) == 0
        assert eng.verify_aggregates_shared(sigs, msgs, index, key_sets, seed=SEEDS[2]) == (True, bytes(n)) == eng.verify_aggregates(sigs, full, key_sets, seed=SEEDS[2])
        assert eng.verify_aggregates_indexed_shared(ks, sigs, msgs, index, idx2, seed=SEEDS[2], per_set=False) == (True, None)
    finally:
        other.close()
        ks.close()


def test_65536_sets_over_64_messages(eng, oracle):
    n, m = 65536, 64
    rnd = random.Random(65536 + 64)
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, n, m)
    full = [msgs[g] for g in index]
    for k in rnd.sample(range(n), 24) + [n - 1]:
        assert oracle.verify(sigs[k], full[k], pks[k], DST) == 1
    assert eng.verify_multiple_shared(sigs, msgs, index, pks) == (True, bytes(n))
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, seed=SEEDS[0]) == eng.verify_multiple(sigs, full, pks, seed=SEEDS[0]) == (True, bytes(n))
    sigs[-1] = sigs[0]
    assert oracle.verify(sigs[-1], full[-1], pks[-1], DST) == 0
    ok, st = eng.verify_multiple_shared(sigs, msgs, index, pks)
    assert not ok and st == bytes(n - 1) + b'\x09'
    assert eng.verify_multiple(sigs, full, pks, seed=SEEDS[0]) == eng.verify_multiple_shared(sigs, msgs, index, pks, seed=SEEDS[0]) == (False, st)
    assert eng.verify_multiple_shared(sigs, msgs, index, pks, per_set=False) == (False, None)


def test_refused_calls(eng, oracle):
    """on a live context: refused, nothing run, and the context works afterwards"""
    lib, h = eng.lib, eng.h
    ok = C.c_int(5)
    sig, pk, msg = ZERO_SIG * 2, ZERO_PK * 2, b'mm'
    off = (C.c_uint32 * 3)(0, 1, 2)
    call = lambda n_msgs, idx, offs=off: lib.nbls_verify_multiple_shared(h, 2, sig, n_msgs, msg, offs, idx, pk, DST, len(DST), None, C.byref(ok), None)   # noqa: E731
    assert call(0, (C.c_uint32 * 2)(0, 0)) == EINVAL
    assert call(3, (C.c_uint32 * 2)(0, 1)) == EINVAL
    assert call(2, (C.c_uint32 * 2)(0, 2)) == EINVAL
    assert call(2, (C.c_uint32 * 2)(1, 1)) == EINVAL
    assert call(2, None) == EINVAL
    assert call(2, (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 3)(0, 2, 1)) == EINVAL
    assert ok.value == 5
    with pytest.raises(Exception, match=r'code %d\b' % EINVAL):
        eng.verify_multiple_shared([ZERO_SIG], [b'a', b'b'], [0], [ZERO_PK])
    want = expected(oracle.verify(ZERO_SIG, b'a', ZERO_PK, DST), ZERO_PK)
    assert want == 1 and eng.verify_multiple_shared([ZERO_SIG], [b'a'], [0], [ZERO_PK], seed=SEEDS[0]) == (False, bytes([want]))


def test_scratch_intact_before_and_after(eng, oracle, golden):
    """a call of another kind before and after a shared call (and the per-set pass in between) gives unchanged results"""
    ms = [b'scratch %d' % i for i in range(8)]
    apk, agg = oracle.aggregate_sign(ms, [bytes([7 + i]) * 32 for i in range(8)])
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:6])
    g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:6])
    want = oracle.pairing_batch(g1, g2, True, False)[0]
    rnd = random.Random(28)
    plain = shared_sets(eng, rnd, 50, 50, list(range(50)))
    full = plain[1]
    before = eng.verify_multiple(plain[0], full, plain[3], seed=SEEDS[0]), eng.verify_batch(agg, ms, apk), eng.pairing_batch(g1, g2, True, False)[0]
    assert before == ((True, bytes(50)), True, want)
    sigs, msgs, index, pks, _ = shared_sets(eng, rnd, 90, 7)
    sigs[3] = sigs[4]
    st = check(eng, oracle, sigs, msgs, index, pks, altered=[3])
    assert st[3] == 9 and sum(st) == 9
    after = eng.verify_multiple(plain[0], full, plain[3], seed=SEEDS[0]), eng.verify_batch(agg, ms, apk), eng.pairing_batch(g1, g2, True, False)[0]
    assert after == before
    assert eng.verify_batch(agg, ms[::-1], apk) is False
