"""Miller products against an exact reference at every grouping the runtime chooses: pairs per accumulator (1 / 2 / 4 / 8), the two halves of a chunk, the unit tables
that pad a partial last group, the chunks of more than LINES_CHUNK pairs, the sub-batches of verifyBatch.  The oracle cannot multiply 10^5 Miller loops in a test's time,
so the large inputs repeat a small base set: B1 G1 points and B2 G2 points (coprime counts), pair i = (i mod B1, (7 i + i // B1) mod B2), which runs through all B1 x B2
combinations every B1 B2 pairs.  The raw Miller value m_ab of each combination comes from the oracle once, and the expected product is prod m_ab ^ count_ab -- exact, independent
of the order of the pairs: a dropped, duplicated or wrongly padded pair changes it."""
import collections
import ctypes as C
import hashlib
import importlib
import json
import os
import random
import subprocess
import sys
import textwrap

import pytest
import torch

import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
B1, B2 = 61, 67
THREADS = min(16, os.cpu_count() or 1)
ONE = bytes(47) + b'\x01' + bytes(528)
ACC = ('acc_raw', 'acc2_raw', 'acc4_raw', 'acc8_raw')


def _idx(n):
    return [(i % B1, (7 * i + i // B1) % B2) for i in range(n)]


def _scalar(tag, i):
    return int.from_bytes(hashlib.sha256(b'nbls-products-%s-%d' % (tag, i)).digest(), 'big') % R or 1


def _pow(oracle, a, e):
    out = C.create_string_buffer(576)
    oracle.lib.oracle_fp12_pow_u64(a, C.c_uint64(e), out)
    return out.raw


def _product(oracle, values, counts, extra=()):
    """prod values[k] ^ counts[k] (times every Fp12 in extra), raw: no final exponentiation"""
    acc = ONE
    for k, c in counts.items():
        acc = oracle.bin('fp12_mul', acc, _pow(oracle, values[k], c), 576)
    for x in extra:
        acc = oracle.bin('fp12_mul', acc, x, 576)
    return acc


def _accs(tm):
    return {k for k in tm if k in ACC}


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


@pytest.fixture(scope='module')
def eng():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)


@pytest.fixture(scope='module')
def base(oracle):
    """B1 G1 points, B2 G2 points and the oracle's raw Miller value of every one of the B1 x B2 combinations"""
    g1, g2 = oracle.g1_generator(), oracle.g2_generator()
    P = [oracle.g1_mul(g1, _scalar(b'p', a))[1] for a in range(B1)]
    Q = [oracle.g2_mul(g2, _scalar(b'q', b))[1] for b in range(B2)]
    keys = [(a, b) for a in range(B1) for b in range(B2)]
    raw, _ = oracle.pairing_batch(b''.join(P[a] for a, _ in keys), b''.join(Q[b] for _, b in keys), False, False, threads=THREADS)
    return P, Q, {k: raw[576 * j:576 * j + 576] for j, k in enumerate(keys)}


def _inputs(base, n):
    P, Q, _ = base
    idx = _idx(n)
    return idx, b''.join(P[a] for a, _ in idx), b''.join(Q[b] for _, b in idx)


# size -> the accumulation program the default tuning runs (None: the fused one-program Miller loop, no line tables)
DEFAULT_SIZES = [
    (4096, None), (4097, 'acc_raw'),                                                          # fused -> two programs
    (6143, 'acc_raw'), (6144, 'acc2_raw'), (6145, 'acc2_raw'),                                # GR 1 -> 2, an odd last group
    (16383, 'acc2_raw'), (16384, 'acc2_raw'), (16385, 'acc2_raw'), (16387, 'acc2_raw'),       # two halves from 16384 pairs; an odd half
    (57343, 'acc2_raw'), (57344, 'acc4_raw'), (57345, 'acc4_raw'), (57347, 'acc4_raw'),       # GR 2 -> 4 (half of the chunk >= 28672); 1..3 unit tables
    (131072, 'acc4_raw'), (131073, 'acc4_raw'), (131075, 'acc4_raw'),                         # a second chunk of 1 and 3 pairs, GR from the first chunk
    ((1 << 18) + 3, 'acc4_raw'),                                                              # BASELINE configs[4] size plus a partial group
]


@pytest.mark.parametrize('n,prog', DEFAULT_SIZES, ids=[str(n) for n, _ in DEFAULT_SIZES])
def test_default_tuning_product(eng, oracle, base, n, prog):
    """miller_product with the library's default tuning, with and without the final exponentiation, equal to the count-based oracle product;
    the accumulation program that ran is the one the size's regime names"""
    idx, G1, G2 = _inputs(base, n)
    exp_raw = _product(oracle, base[2], collections.Counter(idx))
    eng.timing_enable(True)
    try:
        raw = eng.miller_product(G1, G2, False)[0]
        tm_raw = eng.timing_read()
        fe = eng.miller_product(G1, G2, True)[0]
        tm_fe = eng.timing_read()
    finally:
        eng.timing_enable(False)
    want = {prog} if prog else set()
    assert _accs(tm_raw) == want and _accs(tm_fe) == want, (sorted(tm_raw), sorted(tm_fe))
    assert raw == exp_raw
    assert fe == oracle.un('fp12_final_exp', exp_raw, 576)


@pytest.mark.parametrize('n,seed', [(57347, 5), (131073, 6)])
def test_distinct_points_product(eng, oracle, n, seed):
    """n pairwise distinct pairs (k_i G1, c_i G2): the product of their pairings is e(G1, G2)^(sum k_i c_i), the right-hand side from the oracle"""
    rnd = random.Random(seed)
    ks = [rnd.randrange(1, R) for _ in range(n)]
    cs = [rnd.randrange(1, R) for _ in range(n)]
    g1, g2 = oracle.g1_generator(), oracle.g2_generator()
    Pts, st = eng.point_mul_batch([k.to_bytes(32, 'big') for k in ks]); assert not any(st)
    Qts, st = eng.point_mul_batch([c.to_bytes(32, 'big') for c in cs], pts=g2 * n, g2=True); assert not any(st)
    for i in list(range(0, n, 4099)) + [n - 1]:
        assert Pts[96 * i:96 * i + 96] == oracle.g1_mul(g1, ks[i])[1], i
        assert Qts[192 * i:192 * i + 192] == oracle.g2_mul(g2, cs[i])[1], i
    t = sum(k * c for k, c in zip(ks, cs)) % R
    eng.timing_enable(True)
    try:
        got = eng.miller_product(Pts, Qts, True)[0]
        tm = eng.timing_read()
    finally:
        eng.timing_enable(False)
    assert _accs(tm) == {'acc4_raw'}, sorted(tm)
    st, rhs = oracle.pairing(oracle.g1_mul(g1, t)[1], g2)
    assert st == 0 and got == rhs


def _child(script, payload, env, tmp_path, timeout=600):
    """runs `script` in a fresh process (switches read once per process) with `payload` as JSON in a file; -> the JSON the script prints last"""
    src = os.path.join(str(tmp_path), 'payload.json')
    with open(src, 'w') as f:
        json.dump(payload, f)
    head = 'import importlib, json, os, sys\nsys.path.insert(0, %r)\nPAYLOAD = json.load(open(%r))\n' % (ROOT, src)
    r = subprocess.run([sys.executable, '-c', head + textwrap.dedent(script)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


SMALL_SIZES = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 129, 131, 257]
WIDTHS = [(2, 'NBLS_ACC2_MIN', 'acc2_raw'), (4, 'NBLS_ACC4_MIN', 'acc4_raw'), (8, 'NBLS_ACC8_MIN', 'acc8_raw')]


@pytest.mark.parametrize('width,var,prog', WIDTHS, ids=['acc2', 'acc4', 'acc8'])
def test_every_grouping_width(oracle, base, tmp_path, width, var, prog):
    """every pairs-per-accumulator width forced from the first pair (the thresholds are read once per process, hence the child process), two programs at
    every size and two halves from 64 pairs: every residue of n modulo the width in both halves -- equal to oracle.miller_product itself"""
    P, Q, _ = base
    script = '''
        pkg = importlib.import_module('noble-bls12-381_amd')
        eng = pkg.Engine(0)
        eng.set_split_miller_min(0); eng.set_halves_min(64)
        P = [bytes.fromhex(x) for x in PAYLOAD['P']]; Q = [bytes.fromhex(x) for x in PAYLOAD['Q']]
        res = {}
        eng.timing_enable(True)
        for n in PAYLOAD['sizes']:
            idx = [(i % len(P), (7 * i + i // len(P)) % len(Q)) for i in range(n)]
            g1 = b''.join(P[a] for a, _ in idx); g2 = b''.join(Q[b] for _, b in idx)
            raw = eng.miller_product(g1, g2, False)[0]; fe = eng.miller_product(g1, g2, True)[0]
            res[str(n)] = [raw.hex(), fe.hex(), sorted(eng.timing_read())]
        print(json.dumps(res))
    '''
    res = _child(script, {'P': [p.hex() for p in P], 'Q': [q.hex() for q in Q], 'sizes': SMALL_SIZES}, {var: '1'}, tmp_path)
    for n in SMALL_SIZES:
        raw, fe, names = res[str(n)]
        assert _accs(names) == {prog}, (n, names)
        _, G1, G2 = _inputs(base, n)
        assert bytes.fromhex(raw) == oracle.miller_product(G1, G2, False), (n, width)
        assert bytes.fromhex(fe) == oracle.miller_product(G1, G2, True), (n, width)


@pytest.fixture(scope='module')
def signers(oracle):
    """B1 secret keys (compressed and affine public keys), B2 messages (hash points, expand_message_xmd bytes) and the raw Miller value of every (key, hash) combination"""
    sks = [_scalar(b'sk', a) for a in range(B1)]
    pks = [oracle.get_public_key(sk.to_bytes(32, 'big')) for sk in sks]
    pk_aff = [oracle.call('g1_decompress', 96, pk)[1] for pk in pks]
    msgs = [hashlib.sha256(b'nbls-products-msg-%d' % b).digest() for b in range(B2)]
    H = [oracle.hash_to_g2(m)[1] for m in msgs]
    uni = [oracle.expand_message_xmd(m, oracle_py.DST_DEFAULT, 256) for m in msgs]
    keys = [(a, b) for a in range(B1) for b in range(B2)]
    raw, _ = oracle.pairing_batch(b''.join(pk_aff[a] for a, _ in keys), b''.join(H[b] for _, b in keys), False, False, threads=THREADS)
    return dict(sks=sks, pks=pks, msgs=msgs, H=H, uni=uni, values={k: raw[576 * j:576 * j + 576] for j, k in enumerate(keys)},
                neg_g1=oracle.un('g1_neg_aff', oracle.g1_generator(), 96))


def _aggregate(oracle, s, counts):
    """sum_b (sum of the secret keys that sign message b) H(m_b), affine and compressed"""
    per = collections.defaultdict(int)
    for (a, b), c in counts.items():
        per[b] = (per[b] + c * s['sks'][a]) % R
    pts = b''.join(oracle.g2_mul(s['H'][b], k)[1] for b, k in sorted(per.items()) if k)
    zero, aff = oracle.call('g2_sum', 192, C.c_size_t(len(pts) // 192), pts)
    assert not zero
    return aff, oracle.call('g2_compress', 96, aff, C.c_int(0))[1]


def _verify_reference(oracle, s, n):
    """-> (compressed aggregate signature, the raw product verifyBatch multiplies: the n (key, message) pairs and (-G1, S))"""
    counts = collections.Counter(_idx(n))
    sig_aff, sig = _aggregate(oracle, s, counts)
    partial = _product(oracle, s['values'], counts, extra=[oracle.miller_loop(s['neg_g1'], sig_aff)])
    assert oracle.un('fp12_final_exp', partial, 576) == ONE        # the reference is a valid verifyBatch
    return sig, partial


# (signatures, set_verify_pipeline arguments or None for the defaults, sub-batch sizes, accumulation programs)
VERIFY_REGIMES = [
    (4095, None, [4095], set()),                                    # 4096 pairs: the fused Miller loop
    (4096, None, [4096], {'acc_raw'}),
    (6143, None, [6143], {'acc2_raw'}),                             # 6144 pairs
    (6144, None, [6144], {'acc2_raw'}),
    (32767, None, [32767], {'acc2_raw'}),                           # one call: two halves of 16384 pairs
    (32768, None, [24576, 8192], {'acc2_raw'}),                     # the pipeline switches on
    (4095, (2, 50, 0), [2048, 2047], {'acc2_raw'}),                 # the (-G1, S) pair lifts the last sub-batch to 2048 pairs
    (5000, (2, 30, 0), [3520, 1480], {'acc2_raw', 'acc_raw'}),
    (6002, (2, 40, 0), [3648, 2354], {'acc2_raw'}),                 # last: 2355 pairs, one unit table
    (7001, (3, 20, 0), [3328, 2368, 1305], {'acc2_raw', 'acc_raw'}),
    (9004, (4, 10, 0), [3648, 2752, 1856, 748], {'acc2_raw', 'acc_raw'}),
    (70000, (2, 50, 0), [35008, 34992], {'acc4_raw'}),              # last: 34993 pairs, three unit tables
]


@pytest.mark.parametrize('n,tune,plan,progs', VERIFY_REGIMES, ids=['%d-%s' % (n, 'x'.join(map(str, t)) if t else 'default') for n, t, _, _ in VERIFY_REGIMES])
def test_verify_batch_product(eng, oracle, signers, n, tune, plan, progs):
    """verifyBatch's Miller product (nbls_verify_batch_partial_dev: the n pairs and (-G1, S), raw) equal to the count-based reference, in one call and
    cut into 2 / 3 / 4 sub-batches on both sides of the width thresholds; verifyBatch is true, and false when only the last message or only the first
    message of the last sub-batch changes"""
    assert sum(plan) == n
    s = signers
    idx = _idx(n)
    sig, partial = _verify_reference(oracle, s, n)
    if tune:
        eng.set_verify_pipeline(*tune)
    try:
        out = torch.zeros(576, dtype=torch.uint8, device='cuda')
        d_sig, d_uni, d_pk = _dev(sig), _dev(b''.join(s['uni'][b] for _, b in idx)), _dev(b''.join(s['pks'][a] for a, _ in idx))
        eng.timing_enable(True)
        try:
            zero = eng.verify_batch_partial_dev(n, d_sig.data_ptr(), d_uni.data_ptr(), d_pk.data_ptr(), out.data_ptr())
            eng.synchronize()
            tm = eng.timing_read()
        finally:
            eng.timing_enable(False)
        assert not zero
        assert _accs(tm) == progs, sorted(tm)
        assert bytes(out.cpu().numpy().tobytes()) == partial
        msgs = [s['msgs'][b] for _, b in idx]
        pks = [s['pks'][a] for a, _ in idx]
        assert eng.verify_batch(sig, msgs, pks) is True
        last = list(msgs); last[n - 1] = b'another message'
        assert eng.verify_batch(sig, last, pks) is False
        first = list(msgs); first[n - plan[-1]] = b'another message'
        assert eng.verify_batch(sig, first, pks) is False
    finally:
        eng.set_verify_pipeline(2, 25, 32768)


def test_verify_halves_switch(oracle, signers, tmp_path):
    """NBLS_VERIFY_HALVES=1 (off by default): verifyBatch's first sub-batch runs as two halves of whole groups on two streams; forced with four pairs per
    accumulator everywhere (NBLS_VERIFY_ACC4_MIN=1) so that half a sub-batch is not a whole number of groups -- the partial equals the count-based reference"""
    s = signers
    cases = [(1000, (2, 50, 0)), (1001, (3, 30, 0))]
    refs = {n: _verify_reference(oracle, s, n) for n, _ in cases}
    script = '''
        import torch
        pkg = importlib.import_module('noble-bls12-381_amd')
        eng = pkg.Engine(0)
        eng.set_halves_min(64)
        pks = [bytes.fromhex(x) for x in PAYLOAD['pks']]; uni = [bytes.fromhex(x) for x in PAYLOAD['uni']]
        res = {}
        for n, tune, sig in PAYLOAD['cases']:
            idx = [(i % len(pks), (7 * i + i // len(pks)) % len(uni)) for i in range(n)]
            d = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
            d_sig, d_uni, d_pk = d(bytes.fromhex(sig)), d(b''.join(uni[b] for _, b in idx)), d(b''.join(pks[a] for a, _ in idx))
            out = torch.zeros(576, dtype=torch.uint8, device='cuda')
            eng.set_verify_pipeline(*tune)
            eng.timing_enable(True)
            zero = eng.verify_batch_partial_dev(n, d_sig.data_ptr(), d_uni.data_ptr(), d_pk.data_ptr(), out.data_ptr())
            eng.synchronize()
            res[str(n)] = [bytes(out.cpu().numpy().tobytes()).hex(), zero, sorted(eng.timing_read())]
        print(json.dumps(res))
    '''
    payload = {'pks': [p.hex() for p in s['pks']], 'uni': [u.hex() for u in s['uni']], 'cases': [[n, list(t), refs[n][0].hex()] for n, t in cases]}
    res = _child(script, payload, {'NBLS_VERIFY_HALVES': '1', 'NBLS_VERIFY_ACC4_MIN': '1'}, tmp_path)
    for n, _ in cases:
        out, zero, names = res[str(n)]
        assert not zero and _accs(names) == {'acc4_raw'}, (n, names)
        assert bytes.fromhex(out) == refs[n][1], n


def test_pairing_batch_above_one_chunk(eng, oracle, base):
    """131073 pairings (more than LINES_CHUNK: the chunked two-program path), with and without the final exponentiation: every repetition of a combination
    gives the same 576 bytes wherever it sits, and the distinct results equal the oracle's"""
    n = 131073
    idx, G1, G2 = _inputs(base, n)
    P, Q, values = base
    keys = sorted(values)
    fe_ref, _ = oracle.pairing_batch(b''.join(P[a] for a, _ in keys), b''.join(Q[b] for _, b in keys), True, False, threads=THREADS)
    refs = {True: {k: fe_ref[576 * j:576 * j + 576] for j, k in enumerate(keys)}, False: values}
    for fe in (True, False):
        out, st = eng.pairing_batch(G1, G2, fe, False)
        assert st == bytes(n) and len(out) == 576 * n
        ref = refs[fe]
        for i, k in enumerate(idx):
            assert out[576 * i:576 * i + 576] == ref[k], (fe, i)
