"""KZG on the GPU (-m gpu): nbls_fr_eval_roots against Python integers, nbls_kzg_verify_proofs / nbls_kzg_verify_blobs against a test-only trusted setup (kzg_cases.py): with the
secret tau known, C = [p(tau)]G1 and pi = [(p(tau) - y) / (tau - z)]G1 are single multiples of the generator from the oracle, [tau]G2 is the oracle's point compressed by
compress_batch, the challenges come from hashlib.  Nothing expected comes from the calls under test.  The formulas are EIP-4844's as the project's issue states them; the
specification's own vectors are not part of this suite."""
import ctypes as C
import importlib
import random
import pytest
import torch
from goldenio import hx
from kzg_cases import R, M256, LANES, TAU, NOT_VERIFIED, NON_CANONICAL, ZERO48, Setup, b32, roots, eval_roots, blob_bytes, challenge

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))


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
def tau_g2(setup):
    return setup.tau_g2()


@pytest.fixture(scope='module')
def bad_points(golden):
    vec = golden['codec']['g1']
    return {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}


def ints(vals):
    return [int.from_bytes(v, 'big') for v in vals]


# ---- (a) nbls_fr_eval_roots

def structured(log2_n, rnd):
    n, w = 1 << log2_n, roots(log2_n)
    polys = {'random': [rnd.randrange(R) for _ in range(n)], 'zero': [0] * n, 'constant': [rnd.randrange(1, R)] * n, 'X': list(w),
             'r-1': [R - 1 if j == n // 2 else rnd.randrange(R) for j in range(n)]}
    on = sorted({0, n - 1, min(LANES - 1, n - 1), min(LANES, n - 1), max(n - LANES, 0), min(n - LANES + 1, n - 1) if n > LANES else 1})
    points = [('random', rnd.randrange(R)), ('0', 0), ('r-1', R - 1)] + [('w%d' % j, w[j]) for j in on]
    return [(pn + '@' + zn, f, z) for pn, f in polys.items() for zn, z in points]


@pytest.mark.parametrize('log2_n', [2, 8, 12])
def test_eval_roots_structured_cases(eng, log2_n):
    cases = structured(log2_n, random.Random(400 + log2_n))
    got, st = eng.fr_eval_roots(log2_n, [f for _, f, _ in cases], [z for _, _, z in cases])          # one call: z on a root and off it side by side
    assert st == [0] * len(cases)
    for (name, f, z), g in zip(cases, ints(got)):
        assert g == eval_roots(f, z, log2_n), name


@pytest.mark.parametrize('log2_n', [2, 8, 12])
def test_eval_roots_non_canonical_inputs(eng, log2_n):
    rnd = random.Random(410 + log2_n)
    n = 1 << log2_n
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
    zs = [rnd.randrange(R) for _ in range(5)]
    want = [eval_roots(f, z, log2_n) for f, z in zip(fs, zs)]
    fs[1][n - 1] = R
    fs[3][min(LANES + 3, n - 2)] = M256
    got, st = eng.fr_eval_roots(log2_n, fs, zs)
    assert st == [0, NON_CANONICAL, 0, NON_CANONICAL, 0]
    assert ints(got) == [want[0], 0, want[2], 0, want[4]]
    zs[2] = R
    got, st = eng.fr_eval_roots(log2_n, fs, zs)
    assert st == [0, NON_CANONICAL, NON_CANONICAL, NON_CANONICAL, 0]
    assert ints(got) == [want[0], 0, 0, 0, want[4]]


def test_eval_roots_65_polynomials_in_one_call(eng):
    rnd = random.Random(420)
    fs = [[rnd.randrange(R) for _ in range(64)] for _ in range(65)]
    zs = [rnd.randrange(R) if k % 7 else roots(6)[k % 64] for k in range(65)]
    got, st = eng.fr_eval_roots(6, fs, zs)
    assert st == [0] * 65
    assert ints(got) == [eval_roots(f, z, 6) for f, z in zip(fs, zs)]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two or more GPUs')
def test_eval_roots_mainnet_size_on_the_second_device(pkg, eng):
    """N = 4096 asks for 128 KB of dynamic LDS, above the default limit: the raised limit is a per-device attribute of the kernel, so a context on device 1 must get it too --
    after device 0 has made its first launch (the `eng` fixture and the tests above)"""
    rnd = random.Random(425)
    fs = [[rnd.randrange(R) for _ in range(4096)] for _ in range(2)]
    zs = [rnd.randrange(R), roots(12)[4095]]
    want = [eval_roots(f, z, 12) for f, z in zip(fs, zs)]
    got, st = eng.fr_eval_roots(12, fs, zs)
    assert (ints(got), st) == (want, [0, 0])
    other = pkg.Engine(1)
    got, st = other.fr_eval_roots(12, fs, zs)
    assert (ints(got), st) == (want, [0, 0])
    other.close()


# ---- (b) nbls_kzg_verify_proofs, valid and tampered

def tuples(setup, n, rnd, log2_n=2):
    """n valid openings of random polynomials of 2^log2_n values -> lists (commitments, zs, ys, proofs)"""
    cs, zs, ys, ps = [], [], [], []
    for _ in range(n):
        f = [rnd.randrange(R) for _ in range(1 << log2_n)]
        z = rnd.randrange(R)
        y, p = setup.proof(f, z, log2_n)
        cs.append(setup.commit(f, log2_n)); zs.append(z); ys.append(y); ps.append(p)
    return cs, zs, ys, ps


@pytest.fixture(scope='module')
def valid(setup):
    rnd = random.Random(430)
    return {n: tuples(setup, n, rnd) for n in (1, 2, 9, 65)}


@pytest.mark.parametrize('n', [1, 2, 9, 65])
def test_valid_proofs(eng, valid, tau_g2, n):
    cs, zs, ys, ps = valid[n]
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (True, bytes(n))
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=None) == (True, bytes(n))
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED, per_item=False) == (True, None)


@pytest.mark.parametrize('n', [1, 2, 9, 65])
def test_tampered_proofs(eng, setup, valid, tau_g2, n):
    cs, zs, ys, ps = valid[n]
    k = n // 2
    one = bytes(NOT_VERIFIED if i == k else 0 for i in range(n))
    y2 = list(ys); y2[k] = (ys[k] + 1) % R
    assert eng.kzg_verify_proofs(cs, zs, y2, ps, tau_g2, seed=SEED) == (False, one)
    z2 = list(zs); z2[k] = (zs[k] + 1) % R
    assert eng.kzg_verify_proofs(cs, z2, ys, ps, tau_g2, seed=SEED) == (False, one)
    if n >= 2:
        p2 = list(ps); p2[0], p2[n - 1] = ps[n - 1], ps[0]
        assert eng.kzg_verify_proofs(cs, zs, ys, p2, tau_g2, seed=SEED) == (False, bytes(NOT_VERIFIED if i in (0, n - 1) else 0 for i in range(n)))
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, setup.tau_g2(TAU + 1), seed=SEED) == (False, bytes([NOT_VERIFIED]) * n)


# ---- (c) zero points

def test_zero_points_are_valid(eng, setup, valid, tau_g2):
    rnd = random.Random(440)
    cs, zs, ys, ps = [list(v) for v in valid[2]]
    c = rnd.randrange(1, R)
    const = [c] * 4                                   # a constant polynomial: its proof is the zero point
    z = rnd.randrange(R)
    y, p = setup.proof(const, z, 2)
    assert (y, p) == (c, ZERO48)
    assert eng.kzg_verify_proofs(cs + [setup.commit(const, 2)], zs + [z], ys + [y], ps + [p], tau_g2, seed=SEED) == (True, bytes(3))
    assert setup.commit([0] * 4, 2) == ZERO48         # the zero polynomial with y = 0: commitment and proof are the zero point
    assert eng.kzg_verify_proofs(cs + [ZERO48], zs + [z], ys + [0], ps + [ZERO48], tau_g2, seed=SEED) == (True, bytes(3))
    assert eng.kzg_verify_proofs([ZERO48], [z], [0], [ZERO48], tau_g2, seed=SEED) == (True, bytes(1))
    assert eng.kzg_verify_proofs([ZERO48], [z], [1], [ZERO48], tau_g2, seed=SEED) == (False, bytes([NOT_VERIFIED]))


def test_three_constant_polynomials_both_combined_points_zero(eng, setup, tau_g2):
    rnd = random.Random(441)
    vals = [rnd.randrange(1, R) for _ in range(3)]
    cs = [setup.commit([v] * 4, 2) for v in vals]
    zs = [rnd.randrange(R) for _ in range(3)]
    ps = [ZERO48] * 3
    assert eng.kzg_verify_proofs(cs, zs, vals, ps, tau_g2, seed=SEED) == (True, bytes(3))
    assert eng.kzg_verify_proofs(cs, zs, vals, ps, tau_g2, seed=None) == (True, bytes(3))
    wrong = list(vals); wrong[1] = (vals[1] + 5) % R
    assert eng.kzg_verify_proofs(cs, zs, wrong, ps, tau_g2, seed=SEED) == (False, bytes([0, NOT_VERIFIED, 0]))
    assert eng.kzg_verify_proofs(cs, zs, wrong, ps, tau_g2, seed=SEED, per_item=False) == (False, None)


# ---- (d) statuses and return codes

def test_statuses_in_order_and_neighbours_unaffected(eng, valid, tau_g2, bad_points):
    cs, zs, ys, ps = [list(v) for v in valid[9]]
    cs[1] = bad_points['subgroup']                                   # 3
    ps[2] = bad_points['noroot']                                     # 14
    ys[3] = R                                                        # 21
    cs[5] = bad_points['subgroup']; ps[5] = bad_points['noroot']     # the commitment's status comes first
    ps[6] = bad_points['noroot']; zs[6] = M256                       # the proof's before the scalar's
    cs[7] = bad_points['noroot']; ys[7] = R
    want = bytes([0, 3, 14, NON_CANONICAL, 0, 3, 14, 4, 0])
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (False, want)
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED, per_item=False) == (False, None)
    ys[4] = (ys[4] + 1) % R                                          # an invalid tuple among them
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (False, want[:4] + bytes([NOT_VERIFIED]) + want[5:])


def test_return_codes(eng, pkg, valid, tau_g2):
    cs, zs, ys, ps = valid[2]
    args = [b''.join(cs), b''.join(map(b32, zs)), b''.join(map(b32, ys)), b''.join(ps)]
    ok, st = C.c_int32(7), C.create_string_buffer(2)
    lib = eng.lib
    assert lib.nbls_kzg_verify_proofs(eng.h, 2, *args, tau_g2, SEED, C.byref(ok), st) == 0 and ok.value == 1
    bad_tau = bytes([tau_g2[0]]) + bytes(95)                         # x = 0 has no point on the twist with that flag
    for t in (bad_tau, b'\xc0' + bytes(95)):                          # undecodable; the zero point
        ok.value = 7
        assert lib.nbls_kzg_verify_proofs(eng.h, 2, *args, t, SEED, C.byref(ok), st) == -5 and ok.value == 7          # *all_ok is not written on an error
    assert lib.nbls_kzg_verify_proofs(eng.h, 0, *args, tau_g2, SEED, C.byref(ok), st) == -1
    assert lib.nbls_kzg_verify_proofs(eng.h, 2, *args, tau_g2, SEED, C.byref(ok), st) == 0 and ok.value == 1 and st.raw == bytes(2)


# ---- (e) nbls_kzg_verify_blobs, (f) the two calls agree

@pytest.fixture(scope='module')
def blob_cases(setup):
    rnd = random.Random(450)
    out = {}
    for log2_n, n in ((2, 5), (6, 5), (12, 2)):
        out[log2_n] = [setup.blob_case([rnd.randrange(R) for _ in range(1 << log2_n)], log2_n) for _ in range(n)]
    return out


@pytest.mark.parametrize('log2_n', [2, 6, 12])
def test_valid_blobs_and_agreement_with_the_proof_call(eng, blob_cases, tau_g2, log2_n):
    blobs, cs, ps, zs, ys = [list(v) for v in zip(*blob_cases[log2_n])]
    n = len(blobs)
    assert eng.kzg_verify_blobs(log2_n, blobs, cs, ps, tau_g2, seed=SEED) == (True, bytes(n))
    assert eng.kzg_verify_blobs(log2_n, blobs, cs, ps, tau_g2, seed=None) == (True, bytes(n))
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (True, bytes(n))
    # one byte of one blob changed: the challenge and the value move, the proof no longer opens the commitment there
    k = n - 1
    b2 = list(blobs); raw = bytearray(blobs[k]); raw[-1] ^= 1; b2[k] = bytes(raw)
    want = bytes(NOT_VERIFIED if i == k else 0 for i in range(n))
    assert eng.kzg_verify_blobs(log2_n, b2, cs, ps, tau_g2, seed=SEED) == (False, want)
    f2 = [int.from_bytes(b2[k][32 * j:32 * j + 32], 'big') for j in range(1 << log2_n)]
    z2 = challenge(b2[k], cs[k], log2_n)
    zs2, ys2 = list(zs), list(ys); zs2[k], ys2[k] = z2, eval_roots(f2, z2, log2_n)
    assert eng.kzg_verify_proofs(cs, zs2, ys2, ps, tau_g2, seed=SEED) == (False, want)          # the same statuses from the Python-computed (z, y)


def test_blob_with_a_non_canonical_element(eng, blob_cases, tau_g2):
    blobs, cs, ps, zs, ys = [list(v) for v in zip(*blob_cases[6])]
    raw = bytearray(blobs[1]); raw[32 * 17:32 * 18] = b32(R); blobs[1] = bytes(raw)
    assert eng.kzg_verify_blobs(6, blobs, cs, ps, tau_g2, seed=SEED) == (False, bytes([0, NON_CANONICAL, 0, 0, 0]))
