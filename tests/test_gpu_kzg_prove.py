"""The KZG prover on the GPU (-m gpu): nbls_fr_quotient_roots against Python integers (kzg_prove_cases.quotient), the device-resident setup, nbls_kzg_commit_blobs /
nbls_kzg_compute_proofs / nbls_kzg_compute_blob_proofs against kzg_cases.py's test-only trusted setup: with tau known, every expected commitment and proof is a single multiple of
the generator from the oracle, and sum_j q_j L_j(tau) = (p(tau) - y) / (tau - z) makes the device's bytes comparable exactly.  Nothing expected comes from the calls under test;
what they produce is then fed to the verifier."""
import ctypes as C
import importlib
import random
import pytest
from goldenio import hx
from kzg_cases import R, M256, LANES, NON_CANONICAL, ZERO48, Setup, b32, roots, blob_bytes
from kzg_prove_cases import quotient, structured, on_roots, lagrange_setup

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
EINVAL, EDECODE = -1, -5


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
def dev_setup(eng, setup):
    """log2_n -> the device-resident setup of that size, created on first use"""
    made = {}

    def get(log2_n):
        if log2_n not in made:
            made[log2_n] = eng.kzg_setup(log2_n, lagrange_setup(setup, log2_n))
        return made[log2_n]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope='module')
def bad_points(golden):
    vec = golden['codec']['g1']
    return {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}


def ints(vals):
    return [int.from_bytes(v, 'big') for v in vals]


# ---- (a) nbls_fr_quotient_roots

@pytest.mark.parametrize('log2_n', [2, 8, 12])
def test_quotient_structured_cases(eng, log2_n):
    cases = structured(log2_n, random.Random(500 + log2_n))
    ys, qs, st = eng.fr_quotient_roots(log2_n, [f for _, f, _ in cases], [z for _, _, z in cases])          # one call: z on a root and off it side by side
    assert st == [0] * len(cases)
    for (name, f, z), y, q in zip(cases, ints(ys), qs):
        assert (y, ints(q)) == quotient(f, z, log2_n), name


def test_quotient_65_polynomials_in_one_call(eng):
    rnd = random.Random(520)
    fs = [[rnd.randrange(R) for _ in range(64)] for _ in range(65)]
    zs = [rnd.randrange(R) if k % 7 else roots(6)[k % 64] for k in range(65)]
    ys, qs, st = eng.fr_quotient_roots(6, fs, zs)
    assert st == [0] * 65
    assert [(y, ints(q)) for y, q in zip(ints(ys), qs)] == [quotient(f, z, 6) for f, z in zip(fs, zs)]
    assert ys == eng.fr_eval_roots(6, fs, zs)[0]          # y is exactly what nbls_fr_eval_roots returns


def test_quotient_non_canonical_inputs(eng):
    rnd = random.Random(521)
    n = 512
    fs = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
    zs = [rnd.randrange(R), rnd.randrange(R), roots(9)[LANES], roots(9)[3], rnd.randrange(R)]
    want = [quotient(f, z, 9) for f, z in zip(fs, zs)]
    fs[1][LANES + 3] = R
    fs[3][n - 1] = M256
    ys, qs, st = eng.fr_quotient_roots(9, fs, zs)
    assert st == [0, NON_CANONICAL, 0, NON_CANONICAL, 0]
    for k in range(5):
        assert (ints([ys[k]])[0], ints(qs[k])) == ((0, [0] * n) if k in (1, 3) else want[k]), k
    zs[2] = R
    ys, qs, st = eng.fr_quotient_roots(9, fs, zs)
    assert st == [0, NON_CANONICAL, NON_CANONICAL, NON_CANONICAL, 0]
    assert (ints([ys[2]])[0], ints(qs[2])) == (0, [0] * n) and (ints([ys[4]])[0], ints(qs[4])) == want[4]


# ---- (b) the setup

def test_setup_creates_and_reports_its_size(dev_setup):
    for k in (2, 6):
        assert dev_setup(k).log2_n == k


def test_setup_refuses_bad_entries(pkg, eng, setup, bad_points):
    good = lagrange_setup(setup, 2)
    for name, want in (('subgroup', 3), ('noroot', 4)):
        pts = list(good); pts[2] = bad_points[name]
        with pytest.raises(pkg.KzgSetupError) as e:
            eng.kzg_setup(2, pts)
        assert (e.value.code, e.value.status) == (EDECODE, bytes([0, 0, want, 0])), name
    pts = list(good); pts[1] = ZERO48
    with pytest.raises(pkg.KzgSetupError) as e:
        eng.kzg_setup(2, pts)
    assert (e.value.code, e.value.status) == (EDECODE, bytes([0, 1, 0, 0]))
    out = C.c_void_p(7)
    assert eng.lib.nbls_kzg_setup_create(eng.h, 2, b''.join(pts), None, C.byref(out)) == EDECODE and out.value is None          # status == NULL; *out = NULL
    assert eng.lib.nbls_kzg_setup_create(eng.h, 13, b''.join(pts), None, C.byref(out)) == EINVAL


def test_setup_outlives_its_context_and_serves_another(pkg, eng, setup):
    rnd = random.Random(530)
    first = pkg.Engine(0)
    su = first.kzg_setup(6, lagrange_setup(setup, 6))
    first.close()
    f = [rnd.randrange(R) for _ in range(64)]
    got, st = eng.kzg_commit_blobs(su, [blob_bytes(f)])          # the size comes from the setup
    assert (got, st) == ([setup.commit(f, 6)], bytes(1))
    su.close()
    with pytest.raises(pkg.NblsError):
        eng.kzg_commit_blobs(su, [blob_bytes(f)])


# ---- (c) nbls_kzg_commit_blobs

def blob_set(log2_n, rnd):
    n = 1 << log2_n
    c = rnd.randrange(1, R)
    return {'random': [rnd.randrange(R) for _ in range(n)], 'zero': [0] * n, 'constant': [c] * n, 'X': list(roots(log2_n)), 'random2': [rnd.randrange(R) for _ in range(n)]}, c


def proof_cases(log2_n):
    """-> ([(f, z)], c): two polynomials at every listed point, then the constant polynomial c off a root and on one, and the zero polynomial"""
    rnd = random.Random(550 + log2_n)
    fs, c = blob_set(log2_n, rnd)
    w = roots(log2_n)
    points = [rnd.randrange(R), 0, R - 1] + [w[j] for j in on_roots(log2_n)]
    return [(f, z) for z in points for f in (fs['random'], fs['X'])] + [(fs['constant'], rnd.randrange(R)), (fs['constant'], w[1]), (fs['zero'], rnd.randrange(R))], c


@pytest.fixture(scope='module')
def proof_runs(eng, dev_setup):
    """log2_n -> what nbls_kzg_compute_proofs gave for proof_cases(log2_n): checked by (d), fed to the verifier by (f)"""
    memo = {}

    def get(log2_n):
        if log2_n not in memo:
            cases, _ = proof_cases(log2_n)
            memo[log2_n] = eng.kzg_compute_proofs(dev_setup(log2_n), [blob_bytes(f) for f, _ in cases], [z for _, z in cases])
        return memo[log2_n]
    return get


@pytest.fixture(scope='module')
def blob_runs(eng, setup, dev_setup):
    """log2_n -> (the oracle's cases, what nbls_kzg_compute_blob_proofs gave with the commitments given, and with none)"""
    memo = {}

    def get(log2_n):
        if log2_n not in memo:
            fs, _ = blob_set(log2_n, random.Random(570 + log2_n))
            cases = [setup.blob_case(f, log2_n) for f in fs.values()]
            blobs, cs = [c[0] for c in cases], [c[1] for c in cases]
            memo[log2_n] = (cases, eng.kzg_compute_blob_proofs(dev_setup(log2_n), blobs, cs), eng.kzg_compute_blob_proofs(dev_setup(log2_n), blobs))
        return memo[log2_n]
    return get


@pytest.mark.parametrize('log2_n', [2, 6, 9])
def test_commit_blobs(eng, setup, dev_setup, log2_n):
    fs, c = blob_set(log2_n, random.Random(540 + log2_n))
    got, st = eng.kzg_commit_blobs(dev_setup(log2_n), [blob_bytes(f) for f in fs.values()])
    assert st == bytes(len(fs))
    want = {k: setup.commit(f, log2_n) for k, f in fs.items()}
    assert want['zero'] == ZERO48 and want['constant'] == setup.g1(c)          # sum_j L_j = 1
    assert dict(zip(fs, got)) == want


# ---- (d) nbls_kzg_compute_proofs

@pytest.mark.parametrize('log2_n', [2, 6, 9])
def test_compute_proofs(setup, proof_runs, log2_n):
    cases, c = proof_cases(log2_n)
    ps, ys, st = proof_runs(log2_n)
    assert st == bytes(len(cases))
    for k, (f, z) in enumerate(cases):
        y, p = setup.proof(f, z, log2_n)
        assert (ints([ys[k]])[0], ps[k]) == (y, p), k
    assert ps[-3:] == [ZERO48] * 3 and ints(ys[-3:]) == [c, c, 0]          # a constant polynomial: the zero proof, status 0


def test_compute_proofs_non_canonical_items(eng, setup, dev_setup):
    rnd = random.Random(560)
    fs = [[rnd.randrange(R) for _ in range(64)] for _ in range(5)]
    zs = [rnd.randrange(R), rnd.randrange(R), roots(6)[5], rnd.randrange(R), rnd.randrange(R)]
    want = [setup.proof(f, z, 6) for f, z in zip(fs, zs)]
    fs[1][17] = R
    zs[3] = M256
    ps, ys, st = eng.kzg_compute_proofs(dev_setup(6), [blob_bytes(f) for f in fs], zs)
    assert st == bytes([0, NON_CANONICAL, 0, NON_CANONICAL, 0])
    for k in range(5):
        assert (ints([ys[k]])[0], ps[k]) == ((0, bytes(48)) if k in (1, 3) else want[k]), k
    cs, st = eng.kzg_commit_blobs(dev_setup(6), [blob_bytes(f) for f in fs])
    assert st == bytes([0, NON_CANONICAL, 0, 0, 0])
    assert cs == [bytes(48) if k == 1 else setup.commit(f, 6) for k, f in enumerate(fs)]


# ---- (e) nbls_kzg_compute_blob_proofs

@pytest.mark.parametrize('log2_n', [2, 6, 9])
def test_compute_blob_proofs(blob_runs, log2_n):
    cases, given, alone = blob_runs(log2_n)
    blobs, cs, ps, zs, ys = [list(v) for v in zip(*cases)]
    assert given == (cs, ps, bytes(len(cases)))
    assert alone == (cs, ps, bytes(len(cases)))          # commitments48 = NULL: committed first, the same bytes


def test_compute_blob_proofs_with_a_non_canonical_blob(eng, setup, dev_setup):
    rnd = random.Random(575)
    fs = [[rnd.randrange(R) for _ in range(64)] for _ in range(3)]
    blobs, cs, ps, _, _ = [list(v) for v in zip(*[setup.blob_case(f, 6) for f in fs])]
    raw = bytearray(blobs[1]); raw[32 * 63:] = b32(R); blobs[1] = bytes(raw)
    want = ([cs[0], bytes(48), cs[2]], [ps[0], bytes(48), ps[2]], bytes([0, NON_CANONICAL, 0]))
    assert eng.kzg_compute_blob_proofs(dev_setup(6), blobs) == want
    assert eng.kzg_compute_blob_proofs(dev_setup(6), blobs, cs)[1:] == want[1:]


# ---- (f) the round trip through the verifier

def test_round_trip_through_the_verifier(eng, setup, dev_setup, proof_runs, blob_runs, tau_g2):
    cs, zs, ys, ps = [], [], [], []
    for log2_n in (2, 6, 9):
        cases, _ = proof_cases(log2_n)
        keep = [0, 1, 2, 3, len(cases) - 3, len(cases) - 2]
        blobs = [blob_bytes(cases[k][0]) for k in keep]
        got, st = eng.kzg_commit_blobs(dev_setup(log2_n), blobs)          # the device's own commitments
        assert st == bytes(len(keep))
        p, y, _ = proof_runs(log2_n)
        cs += got; zs += [cases[k][1] for k in keep]; ys += [y[k] for k in keep]; ps += [p[k] for k in keep]
    n = len(cs)
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (True, bytes(n))
    y2 = list(ys); y2[1] = ys[1][:-1] + bytes([ys[1][-1] ^ 1])          # one byte of y changed
    assert eng.kzg_verify_proofs(cs, zs, y2, ps, tau_g2, seed=SEED) == (False, bytes(9 if i == 1 else 0 for i in range(n)))
    for log2_n in (2, 6, 9):
        cases, _, (cs, ps, _) = blob_runs(log2_n)
        assert eng.kzg_verify_blobs(log2_n, [c[0] for c in cases], cs, ps, tau_g2, seed=SEED) == (True, bytes(len(cases)))


# ---- (g) the mainnet size

def test_mainnet_size(eng, setup, dev_setup, tau_g2):
    rnd = random.Random(580)
    c = rnd.randrange(1, R)
    fs = [[rnd.randrange(R) for _ in range(4096)], [rnd.randrange(R) for _ in range(4096)], [c] * 4096]
    zs = [rnd.randrange(R), roots(12)[4095], rnd.randrange(R)]
    blobs = [blob_bytes(f) for f in fs]
    su = dev_setup(12)
    cs, st = eng.kzg_commit_blobs(su, blobs)
    assert (cs, st) == ([setup.commit(f, 12) for f in fs], bytes(3)) and cs[2] == setup.g1(c)
    ps, ys, st = eng.kzg_compute_proofs(su, blobs, zs)
    want = [setup.proof(f, z, 12) for f, z in zip(fs, zs)]
    assert (list(zip(ints(ys), ps)), st) == (want, bytes(3)) and ps[2] == ZERO48
    case = setup.blob_case(fs[0], 12)
    assert eng.kzg_compute_blob_proofs(su, blobs[:1]) == ([case[1]], [case[2]], bytes(1))
    assert eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2, seed=SEED) == (True, bytes(3))


# ---- (h) slabs

def test_slabs_give_the_same_bytes(pkg, setup, dev_setup):
    rnd = random.Random(590)
    fs = [[rnd.randrange(R) for _ in range(64)] for _ in range(5)]
    zs = [rnd.randrange(R) for _ in range(4)] + [roots(6)[63]]
    blobs = [blob_bytes(f) for f in fs]
    su = dev_setup(6)
    other = pkg.Engine(0)
    default = (other.kzg_commit_blobs(su, blobs), other.kzg_compute_proofs(su, blobs, zs), other.kzg_compute_blob_proofs(su, blobs))
    assert default[0][0] == [setup.commit(f, 6) for f in fs]
    other.set_msm_batch(slab=1)          # a budget below one group's cost: every blob is a slab of its own
    assert (other.kzg_commit_blobs(su, blobs), other.kzg_compute_proofs(su, blobs, zs), other.kzg_compute_blob_proofs(su, blobs)) == default
    other.close()


def test_return_codes(eng, dev_setup):
    su, lib = dev_setup(2), eng.lib
    blob, z = bytes(128), bytes(32)
    out, y, st = C.create_string_buffer(48), C.create_string_buffer(32), C.create_string_buffer(1)
    assert lib.nbls_kzg_commit_blobs(eng.h, su.h, 0, blob, out, st) == EINVAL
    assert lib.nbls_kzg_commit_blobs(eng.h, su.h, (1 << 20) + 1, blob, out, st) == EINVAL
    assert lib.nbls_kzg_compute_proofs(eng.h, su.h, 1, blob, None, out, y, st) == EINVAL
    assert lib.nbls_kzg_compute_blob_proofs(eng.h, su.h, 1, blob, None, None, out, st) == EINVAL
    assert lib.nbls_kzg_commit_blobs(eng.h, su.h, 1, blob, out, None) == 0 and out.raw == ZERO48          # status == NULL
    assert lib.nbls_kzg_compute_proofs(eng.h, su.h, 1, blob, z, out, y, None) == 0 and out.raw == ZERO48 and y.raw == bytes(32)
