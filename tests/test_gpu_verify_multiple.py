"""nbls_verify_multiple on the GPU (-m gpu): n independent (key, message, signature) sets checked together by a random linear combination, every status against
what the oracle's verify(sig_i, m_i, pk_i) does -- 1 / 0 / -1 (a zero point) / -st (the key's decoder) / -10 - st (the signature's decoder)."""
import hashlib
import importlib
import os
import random
import pytest
from goldenio import hx

pytestmark = pytest.mark.gpu
DST = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'
ZERO_PK = b'\xc0' + bytes(47)
ZERO_SIG = b'\xc0' + bytes(95)
SEEDS = [hashlib.sha256(b'seed %d' % k).digest() for k in range(3)]


@pytest.fixture(scope='module')
def eng():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)


def expected(v, pk):
    """oracle.verify's answer -> the status nbls_verify_multiple reports for the set"""
    if v == 1:
        return 0
    if v == 0:
        return 9
    if v == -1:
        return 1 if pk == ZERO_PK else 11
    return -v


def check(eng, oracle, sigs, msgs, pks, dst=DST, seed=SEEDS[0]):
    exp = [expected(oracle.verify(s, m, p, dst), p) for s, m, p in zip(sigs, msgs, pks)]
    ok, st = eng.verify_multiple(sigs, msgs, pks, dst, seed)
    assert list(st) == exp
    assert ok == all(e == 0 for e in exp)
    ok2, st2 = eng.verify_multiple(sigs, msgs, pks, dst, seed, per_set=False)
    assert st2 is None and ok2 == ok
    return list(st)


@pytest.fixture(scope='module')
def sets(eng, testdata):
    vs = testdata['sign_vectors']
    sks = [hx(v[0]) for v in vs]
    return [hx(v[2]) for v in vs], [hx(v[1]) for v in vs], eng.get_public_keys(sks)


def random_sets(eng, n, rnd, dst=DST):
    r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    sks = [rnd.randrange(1, r).to_bytes(32, 'big') for _ in range(n)]
    msgs = [rnd.getrandbits(64).to_bytes(8, 'big') * (1 + i % 3) for i in range(n)]
    return eng.sign_batch(msgs, sks, dst), msgs, eng.get_public_keys(sks)


def test_reference_sign_vectors(eng, oracle, sets):
    sigs, msgs, pks = sets
    assert len(sigs) == 559
    for k in range(0, 559, 37):
        assert oracle.verify(sigs[k], msgs[k], pks[k]) == 1
    for seed in (SEEDS[0], None):
        ok, st = eng.verify_multiple(sigs, msgs, pks, seed=seed)
        assert ok and st == bytes(559)
        ok, st = eng.verify_multiple(sigs, msgs, pks, seed=seed, per_set=False)
        assert ok and st is None


def test_cancellation_attack(eng, oracle, sets):
    """sig_3 + D and sig_7 - D: the plain sum of the signatures is unchanged, so an unweighted check would accept; the weights do not"""
    sigs, msgs, pks = [list(x[:16]) for x in sets]
    g2 = oracle.g2_generator()
    D = oracle.g2_mul(g2, 0x1234567890abcdef1234567890abcdef)[1]
    negD = oracle.g2_mul(g2, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 - 0x1234567890abcdef1234567890abcdef)[1]
    aff, st = oracle.decompress_batch(b''.join(sigs), g2=True)
    assert st == bytes(16)
    a3 = oracle.g2_sum(aff[3 * 192:4 * 192] + D)[1]
    a7 = oracle.g2_sum(aff[7 * 192:8 * 192] + negD)[1]
    bad = list(sigs)
    bad[3], bad[7] = eng.compress_batch(a3 + a7, g2=True)[:96], eng.compress_batch(a3 + a7, g2=True)[96:]
    aff2, st2 = oracle.decompress_batch(b''.join(bad), g2=True)
    assert st2 == bytes(16)
    assert oracle.g2_sum(aff2)[1] == oracle.g2_sum(aff)[1]
    for seed in SEEDS:
        ok, st = eng.verify_multiple(bad, msgs, pks, seed=seed)
        assert not ok
        assert list(st) == [9 if i in (3, 7) else 0 for i in range(16)]
        ok, st = eng.verify_multiple(bad, msgs, pks, seed=seed, per_set=False)
        assert not ok and st is None


def test_wrong_sets(eng, oracle, sets):
    sigs, msgs, pks = [list(x[:12]) for x in sets]
    sigs[1], sigs[2] = sigs[2], sigs[1]                       # swapped signatures
    msgs[5] = msgs[5] + b'x'                                  # a wrong message
    pks[9] = pks[10]                                          # a wrong key
    st = check(eng, oracle, sigs, msgs, pks)
    assert [i for i, v in enumerate(st) if v] == [1, 2, 5, 9] and all(st[i] == 9 for i in (1, 2, 5, 9))


def test_malformed_inputs(eng, oracle, golden, sets):
    sigs, msgs, pks = [list(x[:10]) for x in sets]
    g1_sub = [hx(v['hex']) for v in golden['codec']['g1'] if 'subgroup' in v['result']][0]
    g1_noroot = [hx(v['hex']) for v in golden['codec']['g1'] if v['result'] == 'Invalid compressed G1 point'][0]
    g2_sub = [hx(v['hex']) for v in golden['codec']['g2'] if 'subgroup' in v['result']][0]
    pks[0] = ZERO_PK                                          # 1
    pks[2] = g1_sub                                           # 3
    pks[4] = g1_noroot                                        # 4
    sigs[5] = ZERO_SIG                                        # 11
    sigs[6] = g2_sub                                          # 13
    pks[8], sigs[8] = ZERO_PK, g2_sub                         # the signature's code wins, as in the reference
    st = check(eng, oracle, sigs, msgs, pks)
    assert st == [1, 0, 3, 0, 4, 11, 13, 0, 13, 0]


@pytest.mark.parametrize('n', [1, 2, 3, 8, 63, 64, 65, 1000, 4097])          # 8: the per-set pass's 8 x 36 vectors cross the first workgroup inside a set
def test_sizes(eng, oracle, n):
    rnd = random.Random(n)
    sigs, msgs, pks = random_sets(eng, n, rnd)
    for k in sorted({0, n // 2, n - 1}):
        assert oracle.verify(sigs[k], msgs[k], pks[k]) == 1
    ok, st = eng.verify_multiple(sigs, msgs, pks, seed=SEEDS[1])
    assert ok and st == bytes(n)
    msgs[-1] = msgs[-1] + b'!'
    assert oracle.verify(sigs[-1], msgs[-1], pks[-1]) == 0
    ok, st = eng.verify_multiple(sigs, msgs, pks, seed=SEEDS[1])
    assert not ok and st == bytes(n - 1) + b'\x09'
    ok, st = eng.verify_multiple(sigs, msgs, pks, seed=SEEDS[1], per_set=False)
    assert not ok and st is None


def test_65536_sets(eng, oracle):
    n = 65536
    rnd = random.Random(65536)
    sigs, msgs, pks = random_sets(eng, n, rnd)
    for k in rnd.sample(range(n), 24) + [n - 1]:
        assert oracle.verify(sigs[k], msgs[k], pks[k]) == 1
    ok, st = eng.verify_multiple(sigs, msgs, pks)
    assert ok and st == bytes(n)
    sigs[-1] = sigs[0]
    assert oracle.verify(sigs[-1], msgs[-1], pks[-1]) == 0
    ok, st = eng.verify_multiple(sigs, msgs, pks)
    assert not ok and st == bytes(n - 1) + b'\x09'


def test_dst(eng, oracle):
    rnd = random.Random(300)
    for dst in (b'MY-OWN-DST-FOR-TESTING', bytes(range(256)) + b'0123456789' * 4 + b'abcd'):
        assert len(dst) in (22, 300)
        sks = [rnd.getrandbits(250).to_bytes(32, 'big') for _ in range(20)]
        msgs = [b'message %d' % i for i in range(20)]
        sigs, pks = [oracle.sign(m, k, dst)[1] for m, k in zip(msgs, sks)], [oracle.get_public_key(k) for k in sks]
        msgs[4] = b'not what was signed'
        sigs[11] = sigs[12]
        st = check(eng, oracle, sigs, msgs, pks, dst)
        assert [i for i, v in enumerate(st) if v] == [4, 11]
        assert eng.verify_multiple(sigs, msgs, pks, dst, SEEDS[2]) == eng.verify_multiple(sigs, msgs, pks, dst, SEEDS[2])
        ok, st2 = eng.verify_multiple(sigs, msgs, pks, dst, None)
        assert not ok and list(st2) == st
        # signed under the default tag: no set verifies under another
        ok, st3 = eng.verify_multiple(sigs, msgs, pks, DST, SEEDS[2])
        assert not ok and set(st3) == {9}


def test_program_on_ahead_of_time_kernel(eng):
    k = eng.lib.nbls_program_count() - 1
    assert eng.lib.nbls_program_name(k).decode() == 'g1_mul64'
    kern = eng.lib.nbls_program_kernel(eng.h, k)
    assert kern is not None and kern.decode().startswith('nbls_aot_'), kern


def test_scratch_intact_after(eng, oracle, golden, sets):
    sigs, msgs, pks = [list(x[:40]) for x in sets]
    sigs[3] = sigs[4]
    ok, st = eng.verify_multiple(sigs, msgs, pks, seed=SEEDS[0])
    assert not ok and st[3] == 9
    # verifyBatch and pairings on the same context still agree with the oracle
    ms = [b'scratch %d' % i for i in range(8)]
    apk, agg = oracle.aggregate_sign(ms, [bytes([7 + i]) * 32 for i in range(8)])
    assert oracle.verify_batch(agg, ms, apk) == 1
    assert eng.verify_batch(agg, ms, apk) is True
    assert eng.verify_batch(agg, ms[::-1], apk) is False
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:6])
    g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:6])
    out, _ = eng.pairing_batch(g1, g2, True, False)
    assert out == oracle.pairing_batch(g1, g2, True, False)[0]
