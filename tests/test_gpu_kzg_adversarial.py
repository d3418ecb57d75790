"""The group side of the KZG verifier and the prover's tails at the inputs their first tests left out (-m gpu).  The test-only tau is known (kzg_cases.py), so every point is a
known multiple of G1 from the oracle: a tuple is pi = [s]G1, C = [c]G1 with the integers z, y, it holds exactly when s tau = c + z s - y, and with a fixed seed the weights r_i
are known too (kzg_cases.weight).  `model` restates the combined check in those integers; every case first asserts that its input reaches the branch it was built for, then
asserts the call's full (all_ok, status) answer, stated beforehand.  Nothing expected comes from the code under test.

  A  sizes 257 and 600 (verifier), 300 blobs (prover): the second trip of kzg_sum_kernel's loop `i += 256`; the second block of agg_fix_zero_kernel (a replaced point at index 256: six threads a point), kzg_item_status_kernel and
     kzg_prove_tail_kernel (a zero proof, a zero product and a status past index 256); the per-item pass -- P_ACC_Q with table_stride = 0, final_exp_pipeline, rlc_is_one --
     on more than 65 items
  B  the zero flags BST[0..2] of the three partial sums of B and the flags of A and B, one row per combination: agg_points_kernel's identity and agg_fix_zero_kernel's
     generator in the combined check, both arms of kzg_item_status_kernel (pz ? xz : !xz && one) with xz = 1 under a non-zero proof (row 6) and xz = 0 under a zero one (row 8)
  C  the weights: an error that cancels in the plain sums is caught under every seed; an error built to cancel under the documented r_i is accepted with that seed -- which
     pins r_i and that one r_i multiplies C_i, z_i pi_i and y_i -- and caught with any other seed and with the seed of the OS
  D  the accepting branch `za && zb` of kzg_pipeline with no member zero; `za && !zb` after one y changes
  E  the 256-bit MSM over the proofs with every scalar equal and every point equal: one run of eight identical points in every window
  F  the order of the statuses of nbls_kzg_verify_blobs: commitment, proof, then the non-canonical blob, where the device evaluation's status (yst) joins; log2_n = 1
  G  the scratch slots: SB_KZG_*, MSM_RLC's slots, ctx->F and SB_MSMB_* between KZG calls of growing size and the other pipelines that own them"""
import collections
import hashlib
import importlib
import random
import types
import pytest
from goldenio import hx
from kzg_cases import R, TAU, NOT_VERIFIED, NON_CANONICAL, ZERO48, Setup, b32, roots, eval_roots, blob_bytes, weight
from kzg_prove_cases import lagrange_setup

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
SEED2 = hashlib.sha256(b'kzg adversarial').digest()

Item = collections.namedtuple('Item', 'c s z y C P')          # C = [c]G1, P = pi = [s]G1: the integers behind the bytes


def valid(setup, s, z, y):
    C, z, y, P = setup.tuple_for(s, z, y)
    return Item((y + s * (TAU - z)) % R, s % R, z, y, C, P)


def forged(setup, c, s, z, y):
    return Item(c % R, s % R, z, y, setup.g1(c), setup.g1(s))


def holds(t):
    return (t.s * TAU - t.c - t.z * t.s + t.y) % R == 0


def model(items, seed):
    """the combined check in integers -> ([sum r_i c_i, sum r_i z_i s_i, -sum r_i y_i is zero], A is zero, B is zero, the check accepts: tau A = B)"""
    r = [weight(seed, i) for i in range(len(items))]
    s1 = sum(ri * t.c for ri, t in zip(r, items)) % R
    s2 = sum(ri * t.z * t.s for ri, t in zip(r, items)) % R
    s3 = -sum(ri * t.y for ri, t in zip(r, items)) % R
    a, b = sum(ri * t.s for ri, t in zip(r, items)) % R, (s1 + s2 + s3) % R
    return [s1 == 0, s2 == 0, s3 == 0], a == 0, b == 0, a * TAU % R == b


def quad(t):
    return (t.C, t.z, t.y, t.P) if isinstance(t, Item) else t


def run(eng, tau_g2, ts, seed=SEED, per_item=True):
    cs, zs, ys, ps = zip(*[quad(t) for t in ts])
    return eng.kzg_verify_proofs(list(cs), list(zs), list(ys), list(ps), tau_g2, seed=seed, per_item=per_item)


def nines(n, at):
    return bytes(NOT_VERIFIED if i in at else 0 for i in range(n))


def check(eng, tau_g2, items, bad, seed=SEED):
    """`bad`: the places that do not hold.  First the input itself, in integers; then the call's answer and the fast verdict"""
    assert {i for i, t in enumerate(items) if not holds(t)} == set(bad)
    if seed is not None:
        assert model(items, seed)[3] == (not bad)
    assert run(eng, tau_g2, items, seed) == (not bad, nines(len(items), bad))
    assert run(eng, tau_g2, items, seed, per_item=False) == (not bad, None)


def with_y(t, y):
    if isinstance(t, Item):
        return t._replace(y=y % R)
    return (t[0], t[1], y % R, t[3])


def with_z(t, z):
    return (t[0], z % R, t[2], t[3])


def build_world(setup, rnd):
    """everything that costs more than a few oracle multiplications, once: 600 pooled tuples; 300 blobs of four values over 24 polynomials with their proofs and commitments;
    the setup's four Lagrange points"""
    w = types.SimpleNamespace(setup=setup)
    w.pooled = setup.tuples_pooled(600, rnd)
    polys = [[rnd.randrange(R) for _ in range(4)] for _ in range(24)]
    fs = [polys[i % 24] for i in range(300)]
    zs = [rnd.randrange(R) for _ in range(300)]
    w.const = rnd.randrange(1, R)
    fs[270] = [w.const] * 4                      # a zero proof past index 256
    zs[280] = roots(2)[3]                        # z on a root
    want = [setup.proof(f, z, 2) for f, z in zip(fs, zs)]
    w.commitments = [setup.commit(f, 2) for f in fs]
    fs[290] = [fs[290][0], R, fs[290][2], fs[290][3]]          # a non-canonical element
    want[290], w.commitments[290] = (0, bytes(48)), bytes(48)
    w.blobs, w.blob_zs = [blob_bytes(f) for f in fs], zs
    w.proofs, w.ys = [p for _, p in want], [b32(y) for y, _ in want]
    w.blob_st = bytes(NON_CANONICAL if i == 290 else 0 for i in range(300))
    w.lagrange = lagrange_setup(setup, 2)
    return w


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


@pytest.fixture(scope='module')
def kz(eng, oracle):
    w = build_world(Setup(oracle, eng), random.Random(800))
    w.tau_g2 = w.setup.tau_g2()
    return w


@pytest.fixture(scope='module')
def dev_setup(eng, kz):
    """log2_n -> the device-resident setup of that size, created on first use"""
    made = {}

    def get(log2_n):
        if log2_n not in made:
            made[log2_n] = eng.kzg_setup(log2_n, lagrange_setup(kz.setup, log2_n))
        return made[log2_n]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope='module')
def bad_points(golden):
    vec = golden['codec']['g1']
    return {'subgroup': [hx(v['hex']) for v in vec if 'subgroup' in v['result']][0], 'noroot': [hx(v['hex']) for v in vec if v['result'] == 'Invalid compressed G1 point'][0]}


# ---- A. sizes

# n -> the places (of a constant polynomial's tuple: pi = O; of a tuple with z = 0), each pair a call of its own: at n = 257 there is one place past the first block
SPECIAL = {257: [(256, None), (None, 256)], 600: [(300, 599)]}


@pytest.mark.parametrize('n', [257, 600])
def test_large_batches(eng, kz, n):
    base = kz.pooled[:n]
    assert run(eng, kz.tau_g2, base) == (True, bytes(n))
    assert run(eng, kz.tau_g2, base, seed=None) == (True, bytes(n))
    assert run(eng, kz.tau_g2, base, per_item=False) == (True, None)
    rnd = random.Random(810 + n)
    for const_at, z0_at in SPECIAL[n]:
        ts = list(base)
        if const_at is not None:
            ts[const_at] = kz.setup.tuple_for(0, rnd.randrange(1, R), rnd.randrange(1, R))
            assert ts[const_at][3] == ZERO48
        if z0_at is not None:
            ts[z0_at] = kz.setup.tuple_for(rnd.randrange(2, R), 0, rnd.randrange(1, R))
        assert run(eng, kz.tau_g2, ts) == (True, bytes(n))
        assert run(eng, kz.tau_g2, ts, seed=None) == (True, bytes(n))
        bad = list(ts)
        bad[256] = with_y(bad[256], bad[256][2] + 1)
        bad[n - 1] = with_z(bad[n - 1], bad[n - 1][1] + 1)          # (at n = 257 the same tuple: its y and its z)
        assert run(eng, kz.tau_g2, bad) == (False, nines(n, {256, n - 1}))
        assert run(eng, kz.tau_g2, bad, per_item=False) == (False, None)
        bad = list(ts)
        bad[0] = with_y(bad[0], bad[0][2] + 1)                       # the per-item pass with the special tuples valid: a zero X and a zero product in the second block
        assert run(eng, kz.tau_g2, bad) == (False, nines(n, {0}))


def test_prover_300_blobs(eng, kz, dev_setup):
    su = dev_setup(2)
    ps, ys, st = eng.kzg_compute_proofs(su, kz.blobs, kz.blob_zs)
    assert st == kz.blob_st
    assert ps[270] == ZERO48 and ps[290] == bytes(48) and ys[270] == b32(kz.const)
    assert (ps, ys) == (kz.proofs, kz.ys)
    cs, st = eng.kzg_commit_blobs(su, kz.blobs)
    assert st == kz.blob_st
    assert cs[270] == kz.setup.g1(kz.const) and cs == kz.commitments


# ---- B. the zero-flag matrix

# row -> what the combined check must see when every tuple is of the row's kind: ([the three partial sums of B are zero], A is zero, B is zero)
ROWS = {1: ([False, True, False], False, False), 2: ([False, False, True], False, False), 3: ([False, True, True], False, False), 4: ([False, True, False], True, True),
        5: ([True, True, True], True, True), 6: ([False, False, False], False, True), 7: ([True, False, True], False, False), 8: ([False, True, False], True, False)}


def kind(setup, row, rnd):
    s, z, y = (rnd.randrange(2, R) for _ in range(3))
    if row <= 5:          # valid
        return valid(setup, *{1: (s, 0, y), 2: (s, z, 0), 3: (s, 0, 0), 4: (0, z, y), 5: (0, z, 0)}[row])
    if row == 6:          # X = C + [z]pi - [y]G1 is the zero point, the proof is not
        return forged(setup, y - z * s, s, z, y)
    if row == 7:
        return forged(setup, 0, s, z, 0)
    return forged(setup, y + rnd.randrange(1, R - 1), 0, z, y)          # row 8: C is neither O nor [y]G1


@pytest.mark.parametrize('row', sorted(ROWS))
def test_zero_flag_matrix(eng, kz, row):
    rnd = random.Random(820 + row)
    ks = [kind(kz.setup, row, rnd) for _ in range(3)]
    plain = valid(kz.setup, *(rnd.randrange(2, R) for _ in range(3)))
    for items, of_kind in (([ks[0]], {0}), (ks, {0, 1, 2}), ([ks[0], plain, ks[1]], {0, 2})):
        n = len(items)
        if len(of_kind) == n:
            assert list(model(items, SEED)[:3]) == list(ROWS[row])
        if row > 5:
            check(eng, kz.tau_g2, items, of_kind)
            continue
        check(eng, kz.tau_g2, items, set())
        assert run(eng, kz.tau_g2, items, seed=None) == (True, bytes(n))
        for k in sorted({0, n - 1}):
            bad = list(items)
            bad[k] = with_y(bad[k], bad[k].y + 1)
            check(eng, kz.tau_g2, bad, {k})


def test_invalid_rows_among_valid_tuples(eng, kz):
    rnd = random.Random(830)
    items = [valid(kz.setup, *(rnd.randrange(2, R) for _ in range(3))) for _ in range(5)]
    items.insert(1, kind(kz.setup, 6, rnd))
    items.insert(5, kind(kz.setup, 8, rnd))
    check(eng, kz.tau_g2, items, {1, 5})
    assert run(eng, kz.tau_g2, items, seed=None) == (False, nines(7, {1, 5}))


# ---- C. cancellation

A_AT, B_AT = 1, 4


@pytest.fixture(scope='module')
def six(kz):
    """six valid tuples; the two at A_AT and B_AT open at the same z"""
    rnd = random.Random(840)
    items = [valid(kz.setup, *(rnd.randrange(2, R) for _ in range(3))) for _ in range(6)]
    t = items[B_AT]
    items[B_AT] = valid(kz.setup, t.s, items[A_AT].z, t.y)
    return items


def shifted(setup, t, d):
    """the same C, z, y with the proof [s + d]G1"""
    return forged(setup, t.c, t.s + d, t.z, t.y)


def test_cancellation_unweighted(eng, kz, six):
    """pi_1 + D and pi_4 - D at one z: sum pi_i and sum [z_i]pi_i are unchanged, so the check without weights would accept; with weights no seed does"""
    d = random.Random(841).randrange(1, R)
    bad = list(six)
    bad[A_AT], bad[B_AT] = shifted(kz.setup, six[A_AT], d), shifted(kz.setup, six[B_AT], -d)
    assert sum(t.s * TAU - t.c - t.z * t.s + t.y for t in bad) % R == 0          # the unweighted check
    for seed in (SEED, SEED2, None):
        check(eng, kz.tau_g2, bad, {A_AT, B_AT}, seed)


def test_cancellation_against_known_weights(eng, kz, six):
    """The attack the NULL seed exists for: who knows the seed knows r_i and can choose errors D and -D r_1 / r_4 whose weighted sum vanishes.  The combined check then
    NECESSARILY accepts -- that it does pins the documented r_i (include/nbls.h) for the tuples' indices in the call and that the one r_i multiplies C_i, [z_i]pi_i and y_i;
    any other seed, the seed of the OS, and the same tuples at other indices reject"""
    d = random.Random(842).randrange(1, R)
    ra, rb = weight(SEED, A_AT), weight(SEED, B_AT)
    bad = list(six)
    bad[A_AT], bad[B_AT] = shifted(kz.setup, six[A_AT], d), shifted(kz.setup, six[B_AT], -d * ra * pow(rb, -1, R))
    assert [holds(t) for t in bad] == [i not in (A_AT, B_AT) for i in range(6)]
    assert model(bad, SEED)[1:] == (False, False, True) and not model(bad, SEED2)[3]
    assert run(eng, kz.tau_g2, bad, SEED) == (True, bytes(6))
    assert run(eng, kz.tau_g2, bad, SEED, per_item=False) == (True, None)
    for seed in (SEED2, None):
        check(eng, kz.tau_g2, bad, {A_AT, B_AT}, seed)
    moved = bad[1:] + bad[:1]
    assert not model(moved, SEED)[3]
    check(eng, kz.tau_g2, moved, {A_AT - 1, B_AT - 1}, SEED)


# ---- D. A = B = O with no member zero

def test_both_combined_points_zero_from_non_zero_members(eng, kz):
    rnd = random.Random(850)
    s0, z0, y0, z1, y1 = (rnd.randrange(2, R) for _ in range(5))
    items = [valid(kz.setup, s0, z0, y0), valid(kz.setup, -weight(SEED, 0) * s0 * pow(weight(SEED, 1), -1, R), z1, y1)]
    assert all(ZERO48 not in (t.C, t.P) for t in items)
    assert model(items, SEED) == ([False, False, False], True, True, True)          # r_0 s_0 + r_1 s_1 = 0, and B = tau A for valid tuples
    assert model(items, SEED2)[1:] == (False, False, True)
    for seed in (SEED, SEED2, None):
        check(eng, kz.tau_g2, items, set(), seed)
    bad = [with_y(items[0], y0 + 1), items[1]]
    assert model(bad, SEED)[1:] == (True, False, False)                              # A is still zero, B is not
    check(eng, kz.tau_g2, bad, {0}, SEED)


# ---- E. equal scalars, equal points

def test_one_proof_eight_times_with_equal_weighted_points(eng, kz):
    rnd = random.Random(860)
    k, s = rnd.randrange(1 << 254, R), rnd.randrange(2, R)
    items = [valid(kz.setup, s, k * pow(weight(SEED, i), -1, R) % R, rnd.randrange(1, R)) for i in range(8)]
    assert len({t.P for t in items}) == 1 and all(weight(SEED, i) * t.z % R == k for i, t in enumerate(items))          # every scalar of the 256-bit MSM is k
    check(eng, kz.tau_g2, items, set())
    check(eng, kz.tau_g2, items, set(), SEED2)
    bad = list(items)
    bad[5] = with_y(bad[5], bad[5].y + 1)
    check(eng, kz.tau_g2, bad, {5})


# ---- F. the statuses of nbls_kzg_verify_blobs

def non_canonical(blob, j):
    raw = bytearray(blob)
    raw[32 * j:32 * j + 32] = b32(R)
    return bytes(raw)


def test_blob_statuses_in_order(eng, kz, bad_points):
    rnd = random.Random(870)
    blobs, cs, ps, _, _ = [list(v) for v in zip(*[kz.setup.blob_case([rnd.randrange(R) for _ in range(64)], 6) for _ in range(5)])]
    assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=SEED) == (True, bytes(5))
    for j, k in ((17, 1), (0, 2), (63, 3)):
        blobs[k] = non_canonical(blobs[k], j)
    for name, st in (('subgroup', 3), ('noroot', 4)):
        cs[1] = bad_points[name]                  # the commitment's status comes first
        ps[2] = bad_points[name]                  # the proof's before the blob's
        want = bytes([0, st, 10 + st, NON_CANONICAL, 0])
        assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=SEED) == (False, want)
        assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=None) == (False, want)
        assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=SEED, per_item=False) == (False, None)


def test_blobs_of_two_elements(eng, kz):
    rnd = random.Random(871)
    blobs, cs, ps, _, _ = [list(v) for v in zip(*[kz.setup.blob_case([rnd.randrange(R) for _ in range(2)], 1) for _ in range(3)])]
    assert eng.kzg_verify_blobs(1, blobs, cs, ps, kz.tau_g2, seed=SEED) == (True, bytes(3))
    assert eng.kzg_verify_blobs(1, blobs, cs, ps, kz.tau_g2, seed=None) == (True, bytes(3))
    raw = bytearray(blobs[1]); raw[31] ^= 1; blobs[1] = bytes(raw)
    assert int.from_bytes(blobs[1][:32], 'big') < R
    assert eng.kzg_verify_blobs(1, blobs, cs, ps, kz.tau_g2, seed=SEED) == (False, bytes([0, NOT_VERIFIED, 0]))
    assert eng.kzg_verify_blobs(1, blobs, cs, ps, kz.tau_g2, seed=SEED, per_item=False) == (False, None)


# ---- G. interplay

def test_scratch_intact_between_kzg_and_the_other_pipelines(pkg, kz, oracle, golden, testdata):
    rnd = random.Random(880)
    eng = pkg.Engine(0)          # a context of its own: every slot starts empty and grows here
    su2, su6 = eng.kzg_setup(2, kz.lagrange), eng.kzg_setup(6, lagrange_setup(kz.setup, 6))
    vs = testdata['sign_vectors'][:64]
    sigs, msgs = [hx(v[2]) for v in vs], [hx(v[1]) for v in vs]
    pks = [oracle.get_public_key(hx(v[0])) for v in vs]
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:7])
    g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:7])
    gen = oracle.g1_generator()
    a = [rnd.randrange(1, R) for _ in range(16)]
    pts = [oracle.g1_mul(gen, x)[1] for x in a]

    def group(n):
        idx, ks = [rnd.randrange(16) for _ in range(n)], [rnd.randrange(1 << 256) for _ in range(n)]
        return b''.join(pts[i] for i in idx), [b32(k) for k in ks], oracle.g1_mul(gen, sum(a[i] * k for i, k in zip(idx, ks)) % R)[1]
    groups, forty = [group(n) for n in (3, 33, 70)], group(40)
    polys, zs = [[rnd.randrange(R) for _ in range(256)] for _ in range(3)], [rnd.randrange(R), roots(8)[255], rnd.randrange(R)]
    six_sigs = sigs[:6]; six_sigs[2] = sigs[3]
    assert oracle.verify(six_sigs[2], msgs[2], pks[2]) == 0 and oracle.verify(sigs[2], msgs[2], pks[2]) == 1

    def recorded():
        return [eng.verify_multiple(six_sigs, msgs[:6], pks[:6], seed=SEED),
                eng.pairing_batch(g1, g2, True, False)[0],
                eng.msm_batch([g[0] for g in groups], [g[1] for g in groups]),
                eng.msm(forty[0], forty[1]),
                eng.fr_eval_roots(8, polys, zs),
                eng.kzg_compute_proofs(su2, kz.blobs[:3], kz.blob_zs[:3])]
    want = [(False, nines(6, {2})),
            oracle.pairing_batch(g1, g2, True, False)[0],
            ([g[2] for g in groups], [0, 0, 0]),
            (forty[2], 0),
            ([b32(eval_roots(f, z, 8)) for f, z in zip(polys, zs)], [0, 0, 0]),
            (kz.proofs[:3], kz.ys[:3], bytes(3))]
    assert recorded() == want
    # KZG and its neighbours in growing sizes: every slot they share regrows between the recorded calls
    assert run(eng, kz.tau_g2, kz.pooled[:2]) == (True, bytes(2))
    bad = list(sigs); bad[40] = sigs[41]
    assert eng.verify_multiple(bad, msgs, pks, seed=SEED) == (False, nines(64, {40}))
    ts = kz.pooled[:300]
    ts[123] = with_y(ts[123], ts[123][2] + 1)
    assert run(eng, kz.tau_g2, ts) == (False, nines(300, {123}))          # the per-item pass
    assert eng.msm_batch([g[0] for g in groups[::-1]], [g[1] for g in groups[::-1]]) == ([g[2] for g in groups[::-1]], [0, 0, 0])
    blobs, cs, ps, _, _ = [list(v) for v in zip(*[kz.setup.blob_case([rnd.randrange(R) for _ in range(64)], 6) for _ in range(4)])]
    assert eng.kzg_compute_blob_proofs(su6, blobs) == (cs, ps, bytes(4))
    assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=SEED) == (True, bytes(4))
    ps[3] = ps[0]
    assert eng.kzg_verify_blobs(6, blobs, cs, ps, kz.tau_g2, seed=SEED) == (False, nines(4, {3}))
    assert recorded() == want
    su2.close(); su6.close()
    eng.close()
