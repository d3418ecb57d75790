"""GPU parity tests of the multi-scalar multiplication (nbls_g1_msm / nbls_g2_msm) against the CPU oracle."""
import hashlib
import importlib
import itertools
import json
import os
import random
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.fixture(scope='module')
def eng():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)


def _points(oracle, n, seed, g2=False):
    """n points a_i * G with known a_i (so that large sums can be checked with ONE oracle multiplication)"""
    gen = oracle.g2_generator() if g2 else oracle.g1_generator()
    mul = oracle.g2_mul if g2 else oracle.g1_mul
    a = [int.from_bytes(hashlib.sha256(b'msm-%d-%d' % (seed, i)).digest(), 'big') % R_ORDER or 1 for i in range(n)]
    return a, [mul(gen, x)[1] for x in a]


def _ref(oracle, a, ks, g2=False):
    gen = oracle.g2_generator() if g2 else oracle.g1_generator()
    t = sum(x * k for x, k in zip(a, ks)) % R_ORDER
    return (oracle.g2_mul if g2 else oracle.g1_mul)(gen, t)[1] if t else None


@pytest.mark.parametrize('n', [1, 2, 3, 33, 500])
def test_g1_msm_vs_oracle(eng, oracle, n):
    rnd = random.Random(n)
    a, pts = _points(oracle, n, n)
    ks = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    out, st = eng.msm(b''.join(pts), [k.to_bytes(32, 'big') for k in ks])
    # the oracle's own sum of scalar multiples (independent of the a_i bookkeeping)
    ref = oracle.g1_sum(b''.join(oracle.g1_mul(p, k % R_ORDER)[1] for p, k in zip(pts, ks) if k % R_ORDER))
    assert st == 0 and out == ref[1]
    assert out == _ref(oracle, a, ks)


@pytest.mark.parametrize('n', [1, 5, 120])
def test_g2_msm_vs_oracle(eng, oracle, n):
    rnd = random.Random(100 + n)
    a, pts = _points(oracle, n, 100 + n, g2=True)
    ks = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    out, st = eng.msm(b''.join(pts), [k.to_bytes(32, 'big') for k in ks], g2=True)
    ref = oracle.g2_sum(b''.join(oracle.g2_mul(p, k % R_ORDER)[1] for p, k in zip(pts, ks) if k % R_ORDER))
    assert st == 0 and out == ref[1]


def test_msm_edge_cases(eng, oracle):
    a, pts = _points(oracle, 40, 7)
    P = b''.join(pts)
    # empty sum, all-zero scalars, k P + k (-P): the zero point (status 1)
    assert eng.msm(b'', [])[1] == 1
    assert eng.msm(P, [bytes(32)] * 40)[1] == 1
    neg = oracle.un('g1_neg_aff', pts[0], 96)
    assert eng.msm(pts[0] + neg, [(12345).to_bytes(32, 'big')] * 2)[1] == 1
    # every point in the same bucket of every window (one run of length n: the segmented sum needs ceil(log2 n) rounds)
    k = 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef
    out, st = eng.msm(P, [k.to_bytes(32, 'big')] * 40)
    assert st == 0 and out == _ref(oracle, a, [k] * 40)
    # short scalars (64 bit: 6 windows), scalars >= r, digits 0 and 4095
    rnd = random.Random(5)
    ks = [rnd.randrange(0, 1 << 64) for _ in range(40)]
    out, st = eng.msm(P, [x.to_bytes(32, 'big') for x in ks])
    assert st == 0 and out == _ref(oracle, a, ks)
    ks = [R_ORDER, R_ORDER + 1, (1 << 256) - 1, 0xfff, 0xfff000, 1] + [rnd.randrange(0, 1 << 256) for _ in range(34)]
    out, st = eng.msm(P, [x.to_bytes(32, 'big') for x in ks])
    assert st == 0 and out == _ref(oracle, a, ks)


def test_msm_large_linear(eng, oracle):
    """65,536 points (64 distinct base points a_j G repeated with different scalars): the result must be
    (sum_i a_i k_i mod r) G -- one oracle multiplication; and linearity: msm(P, k) + msm(P, k') == msm(P, k + k')"""
    n = 65536
    a64, p64 = _points(oracle, 64, 99)
    rnd = random.Random(65536)
    a = [a64[i % 64] for i in range(n)]
    P = b''.join(p64) * (n // 64)
    k1 = [rnd.randrange(0, R_ORDER) for _ in range(n)]
    k2 = [rnd.randrange(0, R_ORDER) for _ in range(n)]
    o1, s1 = eng.msm(P, [k.to_bytes(32, 'big') for k in k1])
    o2, s2 = eng.msm(P, [k.to_bytes(32, 'big') for k in k2])
    o3, s3 = eng.msm(P, [((x + y) % R_ORDER).to_bytes(32, 'big') for x, y in zip(k1, k2)])
    assert s1 == 0 and s2 == 0 and s3 == 0
    assert o1 == _ref(oracle, a, k1) and o2 == _ref(oracle, a, k2)
    assert oracle.g1_sum(o1 + o2)[1] == o3
    # G2 at 4096
    n2 = 4096
    b64, q64 = _points(oracle, 64, 98, g2=True)
    kk = [rnd.randrange(0, R_ORDER) for _ in range(n2)]
    o, s = eng.msm(b''.join(q64) * (n2 // 64), [k.to_bytes(32, 'big') for k in kk], g2=True)
    assert s == 0 and o == _ref(oracle, [b64[i % 64] for i in range(n2)], kk, g2=True)


# ---- every scalar-width path of dev_msm (csrc/pipelines_msm.cpp) and the edges of the bucket kernels (csrc/msm_kernels.hip) --------------------------------------------
# dev_msm takes nbits from the caller (msm_host: the longest scalar's bit length): up to 192 bits it runs unsplit with ceil(nbits / 12) windows (1 .. 16), above it splits
# along the endomorphisms into 129-bit (G1, 11 windows) or 65-bit (G2, 6 windows) digits.  References: the oracle and Python integers only.
P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
Z = 0xd201000000010000
BIT_LENGTHS = [1, 11, 12, 13, 24, 64, 65, 128, 129, 180, 181, 191, 192, 193, 254, 255, 256]
DIGIT_EDGES = [Z ** 2 - 1, Z ** 2, Z ** 3, Z ** 4 - 1, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, Z ** 2 * ((1 << 129) - 1) % (1 << 256)]
K64 = 0x9abcdef123456789      # every one of its six 12-bit digits is non-zero: 0x789, 0x456, 0x123, 0xdef, 0xabc, 0x9


def _b32(ks):
    return [k.to_bytes(32, 'big') for k in ks]


def _neg(pt):
    """the negative of an affine wire point of G1 (96 B) or G2 (192 B): every coordinate of y -> p - y"""
    h = len(pt) // 2
    return pt[:h] + b''.join(((P_MOD - int.from_bytes(pt[i:i + 48], 'big')) % P_MOD).to_bytes(48, 'big') for i in range(h, 2 * h, 48))


def _sum_of_multiples(oracle, pts, ks, g2=False):
    """the oracle's own g*_sum of its g*_mul results (no a_i bookkeeping); None for the zero point"""
    mul, add = (oracle.g2_mul, oracle.g2_sum) if g2 else (oracle.g1_mul, oracle.g1_sum)
    terms = b''.join(mul(p, k % R_ORDER)[1] for p, k in zip(pts, ks) if k % R_ORDER)
    zero, out = add(terms)
    return None if zero else out


def _width_scalars(L, n, rnd):
    """n scalars below 2^L: 2^L - 1 (every digit 4095), 2^(L - 1) (the top bit alone), 1, the rest random"""
    return [(1 << L) - 1, 1 << (L - 1), 1] + [rnd.randrange(0, 1 << L) for _ in range(n - 3)]


@pytest.fixture(scope='module')
def widths(oracle):
    """the cases of the width matrix and of the split path's digit edges, computed once: {'g1' | 'g2': (points, [(label, scalars, expected bytes)])}.  Expected = one oracle
    multiplication by sum a_i k_i mod r, checked here against the oracle's sum of its own multiples"""
    out = {}
    for g2 in (False, True):
        a, pts = _points(oracle, 9, 200 + g2, g2=g2)
        rnd = random.Random(300 + g2)
        cases = [('L%d' % L, _width_scalars(L, 7, rnd)) for L in BIT_LENGTHS] + [('edges', DIGIT_EDGES)]
        done = []
        for label, ks in cases:
            assert all(0 <= k < (1 << 256) for k in ks)
            exp = _ref(oracle, a, ks, g2=g2)
            assert exp is not None and exp == _sum_of_multiples(oracle, pts, ks, g2=g2), (g2, label)
            done.append((label, ks, exp))
        out['g2' if g2 else 'g1'] = (pts, done)
    return out


@pytest.mark.parametrize('grp', ['g1', 'g2'])
def test_msm_bit_length_matrix(eng, widths, grp):
    """n = 7 at every bit length on both sides of a window boundary (12 / 13, 24, 64 / 65, 128 / 129, 180 / 181), at 1 and 16 windows (L = 1, 11, 191, 192), on both sides of the
    switch to the endomorphism split (192 / 193) and at 254 .. 256 bits; then the split path's digit edges: multiples and neighbours of z^2, r - 1, r, r + 1, 2^256 - 1"""
    pts, cases = widths[grp]
    for label, ks, exp in cases:
        out, st = eng.msm(b''.join(pts[:len(ks)]), _b32(ks), g2=grp == 'g2')
        assert st == 0 and out == exp, (grp, label)


def _child(script, payload, env, tmp_path, timeout=300):
    """`script` in a fresh process (the switches are read once per process) with `payload` as JSON in a file -> the JSON it prints last"""
    src = os.path.join(str(tmp_path), 'payload.json')
    with open(src, 'w') as f:
        json.dump(payload, f)
    head = 'import importlib, json, os, sys\nsys.path.insert(0, %r)\nPAYLOAD = json.load(open(%r))\n' % (ROOT, src)
    r = subprocess.run([sys.executable, '-c', head + textwrap.dedent(script)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_g1_msm_tail_as_step_programs(widths, tmp_path):
    """NBLS_MSM_WIDE=0: the tail of the G1 sum runs as the step programs g1_horner / g1_shiftadd instead of the one-wavefront combine kernel -- the same expected bytes at every
    width and digit edge; the programs that ran are named by the timing table"""
    pts, cases = widths['g1']
    script = '''
        import torch
        pkg = importlib.import_module('noble-bls12-381_amd')
        eng = pkg.Engine(0)
        pts = [bytes.fromhex(x) for x in PAYLOAD['pts']]
        res = []
        eng.timing_enable(True)
        for ks in PAYLOAD['cases']:
            out, st = eng.msm(b''.join(pts[:len(ks)]), [int(k).to_bytes(32, 'big') for k in ks])
            res.append([out.hex(), st, sorted(eng.timing_read())])
        print(json.dumps({'res': res, 'config': eng.config_describe()}))
    '''
    got = _child(script, {'pts': [p.hex() for p in pts], 'cases': [[str(k) for k in ks] for _, ks, _ in cases]}, {'NBLS_MSM_WIDE': '0'}, tmp_path)
    assert 'NBLS_MSM_WIDE=0' in got['config'], got['config']
    for (label, ks, exp), (out, st, names) in zip(cases, got['res']):
        assert st == 0 and bytes.fromhex(out) == exp, label
        assert 'g1_horner' in names, (label, names)
        assert ('g1_shiftadd' in names) == (label != 'L1' and label != 'L11' and label != 'L12'), (label, names)     # one window: nothing to shift


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize('grp', ['g1', 'g2'])
def test_msm_dev_every_nbits(eng, oracle, grp):
    """nbls_msm_dev on device buffers: 33 points with 64-bit scalars give the oracle's bytes whatever bound nbits the caller states (6, 8, 9 and 16 windows, the split path from
    193 bits, 0 and anything over 256 meaning 256), on the context's stream and on a caller's; result and status land in buffers pre-filled with 0x7f; n = 0 is the zero point"""
    g2 = grp == 'g2'
    n, sz = 33, 192 if g2 else 96
    a, pts = _points(oracle, n, 400 + g2, g2=g2)
    rnd = random.Random(401 + g2)
    ks = [(1 << 64) - 1, 1 << 63, 1] + [rnd.randrange(0, 1 << 64) for _ in range(n - 3)]
    exp = _ref(oracle, a, ks, g2=g2)
    assert exp is not None
    d_pts, d_ks = _dev(b''.join(pts)), _dev(b''.join(_b32(ks)))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        for stream in (0, side.cuda_stream):
            for nbits in (64, 65, 96, 100, 192, 193, 255, 0, 256, 300):
                d_out = torch.full((sz,), 0x7f, dtype=torch.uint8, device='cuda'); d_st = torch.full((1,), 0x7f, dtype=torch.uint8, device='cuda')
                torch.cuda.synchronize()
                eng.msm_dev(g2, n, d_pts.data_ptr(), d_ks.data_ptr(), nbits, d_out.data_ptr(), d_st.data_ptr(), stream=stream)
                eng.synchronize(); torch.cuda.synchronize()
                assert _host(d_st) == b'\0' and _host(d_out) == exp, (grp, nbits, stream != 0)
            d_st = torch.full((1,), 0x7f, dtype=torch.uint8, device='cuda'); d_out = torch.full((sz,), 0x7f, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            eng.msm_dev(g2, 0, None, None, 64, d_out.data_ptr(), d_st.data_ptr(), stream=stream)
            eng.synchronize(); torch.cuda.synchronize()
            assert _host(d_st) == b'\1', (grp, stream != 0)
    finally:
        torch.cuda.synchronize()      # every stream is idle before the buffers go


@pytest.fixture(scope='module')
def base64pts(oracle):
    return {False: _points(oracle, 64, 500), True: _points(oracle, 64, 501, g2=True)}


LONG_RUNS = [('g1', 255), ('g1', 256), ('g1', 257), ('g1', 4096), ('g1', 4097), ('g1', 8193), ('g2', 4097)]


@pytest.mark.parametrize('grp,n', LONG_RUNS, ids=['%s-%d' % c for c in LONG_RUNS])
def test_msm_one_long_run(eng, oracle, base64pts, grp, n):
    """every scalar 1: one window, ONE run of n equal keys -- ceil(log2 n) rounds of the segmented sum (the round loop is d < maxrun: 2^k and 2^k + 1 differ by a round), runs that
    end at, before and behind a 256-thread block of the rank kernel and pairs that reach across msm_pairs_kernel's 4096-element workgroup.  Reference: the oracle's sum"""
    g2 = grp == 'g2'
    a, p64 = base64pts[g2]
    P = b''.join(p64[i % 64] for i in range(n))
    zero, exp = (oracle.g2_sum if g2 else oracle.g1_sum)(P)
    assert not zero
    out, st = eng.msm(P, [(1).to_bytes(32, 'big')] * n, g2=g2)
    assert st == 0 and out == exp
    assert out == _ref(oracle, [a[i % 64] for i in range(n)], [1] * n, g2=g2)


def test_msm_six_long_runs(eng, oracle, base64pts):
    """one 64-bit scalar shared by 4097 points, every 12-bit digit non-zero: six runs of 4097 sorted keys whose boundaries fall inside the workgroups of the pairs kernel"""
    n = 4097
    a, p64 = base64pts[False]
    P = b''.join(p64[i % 64] for i in range(n))
    zero, total = oracle.g1_sum(P)
    assert not zero
    out, st = eng.msm(P, [K64.to_bytes(32, 'big')] * n)
    assert st == 0 and out == oracle.g1_mul(total, K64)[1]


@pytest.mark.parametrize('grp', ['g1', 'g2'])
def test_msm_inside_one_bucket(eng, oracle, grp):
    """one scalar k for every point, so in every window all of them share a bucket: [P, -P, Q] takes the bucket through the zero point (result [k]Q), [P, P, Q] doubles by the
    addition program (result [k](2P + Q)), in every order of the three points, unsplit (64-bit k) and split (255-bit k); [P, -P, Q, -Q] plus ten points with scalar 0 is the
    zero point while the list is not empty"""
    g2 = grp == 'g2'
    _, pts = _points(oracle, 12, 600 + g2, g2=g2)
    P, Q = pts[0], pts[1]
    mul, add = (oracle.g2_mul, oracle.g2_sum) if g2 else (oracle.g1_mul, oracle.g1_sum)
    zero, p2q = add(P + P + Q)
    assert not zero and add(P + _neg(P))[0] == 1      # (the Python negation is the oracle's)
    for k in (K64, (1 << 254) + 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef):
        kq, kp2q = mul(Q, k % R_ORDER)[1], mul(p2q, k % R_ORDER)[1]
        for order in itertools.permutations(range(3)):
            cancel, double = [P, _neg(P), Q], [P, P, Q]
            out, st = eng.msm(b''.join(cancel[i] for i in order), _b32([k] * 3), g2=g2)
            assert st == 0 and out == kq, (grp, k.bit_length(), order, 'cancel')
            out, st = eng.msm(b''.join(double[i] for i in order), _b32([k] * 3), g2=g2)
            assert st == 0 and out == kp2q, (grp, k.bit_length(), order, 'double')
        out, st = eng.msm(b''.join([P, _neg(P), Q, _neg(Q)] + pts[2:12]), _b32([k] * 4 + [0] * 10), g2=g2)
        assert st == 1, (grp, k.bit_length())
