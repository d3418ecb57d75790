"""GPU parity tests of the batched multi-scalar multiplication (nbls_g*_msm_batch / nbls_g*_msm_rows, csrc/pipelines_msm.cpp) against the CPU oracle.  Every call is checked
twice: against the oracle (its own sum of scalar multiples for small groups, the a_i G bookkeeping of test_gpu_msm.py -- one oracle multiplication per group -- for larger
ones), and byte for byte against eng.msm on every group alone."""
import ctypes as C
import hashlib
import importlib
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
WIDTHS = [4, 6, 8, 10, 12]
EINVAL = -1


@pytest.fixture(scope='module')
def engine():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_msm_batch(window=0, big=0, slab=0)


@pytest.fixture(scope='module')
def pool(oracle):
    """64 G1 and 16 G2 points a_i G with known a_i, computed once: the groups of every test draw from them"""
    def make(n, g2):
        gen = oracle.g2_generator() if g2 else oracle.g1_generator()
        mul = oracle.g2_mul if g2 else oracle.g1_mul
        a = [int.from_bytes(hashlib.sha256(b'msmb-%d-%d' % (g2, i)).digest(), 'big') % R_ORDER or 1 for i in range(n)]
        return a, [mul(gen, x)[1] for x in a]
    return {False: make(64, False), True: make(16, True)}


def b32(ks):
    return [k.to_bytes(32, 'big') for k in ks]


def neg(pt):
    h = len(pt) // 2
    return pt[:h] + b''.join(((P_MOD - int.from_bytes(pt[i:i + 48], 'big')) % P_MOD).to_bytes(48, 'big') for i in range(h, 2 * h, 48))


def draw(pool, g2, n, rnd):
    """n points of the pool (with repeats) -> (their a_i, their wire bytes)"""
    a, pts = pool[g2]
    idx = [rnd.randrange(len(a)) for _ in range(n)]
    return [a[i] for i in idx], [pts[i] for i in idx]


def want_of(oracle, a, pts, ks, g2):
    """(wire bytes, status) of sum [k_i]P_i: by the a_i (one oracle multiplication), and for groups of at most 40 points also the oracle's own sum of its multiples"""
    sz = 192 if g2 else 96
    gen = oracle.g2_generator() if g2 else oracle.g1_generator()
    mul, add = (oracle.g2_mul, oracle.g2_sum) if g2 else (oracle.g1_mul, oracle.g1_sum)
    t = sum(x * k for x, k in zip(a, ks)) % R_ORDER
    w = (mul(gen, t)[1], 0) if t else (bytes(sz), 1)
    if len(ks) <= 40:
        zero, out = add(b''.join(mul(p, k % R_ORDER)[1] for p, k in zip(pts, ks) if k % R_ORDER))
        assert ((bytes(sz), 1) if zero else (out, 0)) == w
    return w


def check_batch(eng, oracle, groups, g2=False, alone=True):
    """groups: a list of (a, pts, ks).  One msm_batch call against the oracle and against msm on every group alone; returns the call's outputs"""
    out, st = eng.msm_batch([b''.join(p) for _, p, _ in groups], [b32(k) for _, _, k in groups], g2=g2)
    assert len(out) == len(groups) and len(st) == len(groups)
    for g, (a, pts, ks) in enumerate(groups):
        assert (out[g], st[g]) == want_of(oracle, a, pts, ks, g2), (g, len(ks))
        if alone:
            assert (out[g], st[g]) == eng.msm(b''.join(pts), b32(ks), g2=g2), (g, len(ks))
    return out, st


@pytest.fixture(scope='module')
def mixed(pool):
    rnd = random.Random(1)
    groups = []
    for n in [0, 1, 2, 3, 33, 0, 500, 1]:
        a, pts = draw(pool, False, n, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(n)]))
    return groups


@pytest.mark.parametrize('width', [0] + WIDTHS)
def test_g1_mixed_group_sizes(eng, oracle, mixed, width):
    eng.set_msm_batch(window=width)
    out, st = check_batch(eng, oracle, mixed)
    assert st == [1, 0, 0, 0, 0, 1, 0, 0] and out[0] == bytes(96) and out[5] == bytes(96)


@pytest.mark.parametrize('width', [0, 6, 12])
def test_g2_mixed_group_sizes(eng, oracle, pool, width):
    rnd = random.Random(2)
    groups = []
    for n in [0, 1, 5, 120]:
        a, pts = draw(pool, True, n, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(n)]))
    eng.set_msm_batch(window=width)
    out, st = check_batch(eng, oracle, groups, g2=True)
    assert st == [1, 0, 0, 0] and out[0] == bytes(192)


@pytest.mark.parametrize('width', [0, 4, 12])
def test_group_boundaries(eng, oracle, pool, width):
    """neighbouring groups whose keys agree in window and digit must not meet in one run: equal groups give the single sum each, not a multiple of it"""
    eng.set_msm_batch(window=width)
    rnd = random.Random(3)
    a, pts = draw(pool, False, 9, rnd)
    ks = [rnd.randrange(0, 1 << 256) for _ in range(9)]
    same = (a, pts, ks)
    a2, pts2 = draw(pool, False, 5, rnd)
    other = (a2, pts2, [rnd.randrange(0, 1 << 256) for _ in range(5)])
    single = want_of(oracle, a, pts, ks, False)
    out, st = check_batch(eng, oracle, [other, same, same, other, same, same, same, other])
    assert [(out[g], st[g]) for g in (1, 2, 4, 5, 6)] == [single] * 5 and single[1] == 0
    assert out[0] == out[3] == out[7] and out[0] != out[1]
    # an all-zero group, {P, -P} with equal scalars, and one run of the group's length, each between ordinary neighbours
    zeros = (a2, pts2, [0] * 5)
    k = rnd.randrange(1, R_ORDER)
    cancel = ([a[0], R_ORDER - a[0]], [pts[0], neg(pts[0])], [k, k])
    a3, pts3 = draw(pool, False, 40, rnd)
    one_run = (a3, pts3, [0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef] * 40)
    out2, st2 = check_batch(eng, oracle, [other, zeros, same, cancel, other, one_run, same])
    assert st2 == [0, 1, 0, 1, 0, 0, 0] and out2[1] == bytes(96) and out2[3] == bytes(96)
    assert out2[0] == out2[4] == out[0] and out2[2] == out2[6] == single[0]


@pytest.mark.parametrize('width', [0] + WIDTHS)
def test_scalar_shapes(eng, oracle, pool, width):
    eng.set_msm_batch(window=width)
    c = width or 4
    rnd = random.Random(40 + width)
    top = (1 << c) - 1
    # every scalar of the call below 2^64: no split, ceil(64 / c) windows; digits 0 and 2^c - 1 in every place
    short = [(1 << 64) - 1, top, top << c, 1 << c, 0, 1, top << (c * (63 // c)) & ((1 << 64) - 1)]
    groups = []
    for n in (7, 3, 20):
        a, pts = draw(pool, False, n, rnd)
        groups.append((a, pts, (short + [rnd.randrange(0, 1 << 64) for _ in range(n)])[:n]))
    check_batch(eng, oracle, groups)
    # wide scalars: multiples of r, r + 1, the largest value, small digits at both ends of a window
    wide = [R_ORDER, R_ORDER + 1, (1 << 256) - 1, 2 * R_ORDER, top, top << c, (1 << 256) - (1 << c), 1, 0]
    groups = []
    for n in (9, 2, 1, 30):
        a, pts = draw(pool, False, n, rnd)
        groups.append((a, pts, (wide + [rnd.randrange(0, 1 << 256) for _ in range(n)])[:n]))
    groups.append((groups[0][0][:1], groups[0][1][:1], [R_ORDER]))      # [r]P alone: the zero point
    out, st = check_batch(eng, oracle, groups)
    assert st[-1] == 1


def test_first_offset_above_zero(eng, oracle, pool):
    """the entries in front of the first offset are not read: poison there (bytes that are no point at all, scalars of all ones) changes nothing"""
    rnd = random.Random(5)
    sizes = [4, 0, 11]
    groups = []
    for n in sizes:
        a, pts = draw(pool, False, n, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(n)]))
    want, want_st = check_batch(eng, oracle, groups)
    lead = 6
    P = b'\xff' * (96 * lead) + b''.join(b''.join(p) for _, p, _ in groups)
    K = b'\xff' * (32 * lead) + b''.join(b''.join(b32(k)) for _, _, k in groups)
    offs = (C.c_uint32 * 4)(lead, lead + 4, lead + 4, lead + 15)
    out, st = C.create_string_buffer(96 * 3), C.create_string_buffer(3)
    assert eng.lib.nbls_g1_msm_batch(eng.h, 3, offs, P, K, out, st) == 0
    assert [out.raw[96 * g:96 * g + 96] for g in range(3)] == want and list(st.raw) == want_st
    # status may be NULL
    out2 = C.create_string_buffer(96 * 3)
    assert eng.lib.nbls_g1_msm_batch(eng.h, 3, offs, P, K, out2, None) == 0 and out2.raw == out.raw


@pytest.mark.parametrize('g2', [False, True])
def test_big_group_routing(eng, oracle, pool, g2):
    """a group above the cut-off (forced to 64 points) runs through the single-sum pipeline between the slabs of its small neighbours; two big groups side by side"""
    eng.set_msm_batch(big=64)
    rnd = random.Random(6 + g2)
    groups = []
    for n in ([3, 64, 65, 1, 0, 200, 90, 2] if not g2 else [2, 70, 3]):
        a, pts = draw(pool, g2, n, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(n)]))
    check_batch(eng, oracle, groups, g2=g2)


def test_slabs(eng, oracle, pool):
    """40 groups under a slab budget that holds about twelve of them: at least three slabs, and a group larger than the budget as a slab of its own"""
    rnd = random.Random(8)
    groups = []
    for g in range(40):
        n = 100 if g == 17 else rnd.randrange(0, 9)
        a, pts = draw(pool, False, n, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(n)]))
    want = check_batch(eng, oracle, groups)
    # width 4 on 129-bit halves: 33 windows; a group of n points costs 2 n * 33 + 33 * 4 * 8 = 66 n + 1056 entries, so 16,000 entries hold between 10 and 15 groups of 0 .. 8 points
    eng.set_msm_batch(window=4, slab=16000)
    assert check_batch(eng, oracle, groups) == want
    eng.set_msm_batch(window=8, slab=1)      # every group a slab of its own
    assert check_batch(eng, oracle, groups[:12]) == (want[0][:12], want[1][:12])


def rows_case(eng, oracle, pool, n_pts, n_rows, g2, seed):
    rnd = random.Random(seed)
    a, pts = draw(pool, g2, n_pts, rnd)
    rows = [[rnd.randrange(0, 1 << 256) for _ in range(n_pts)] for _ in range(n_rows)]
    out, st = eng.msm_rows(b''.join(pts), [b32(r) for r in rows], g2=g2)
    assert len(out) == n_rows
    for r in range(n_rows):
        assert (out[r], st[r]) == want_of(oracle, a, pts, rows[r], g2), r
        assert (out[r], st[r]) == eng.msm(b''.join(pts), b32(rows[r]), g2=g2), r
    # the same sums as groups that repeat the points
    assert (out, st) == eng.msm_batch([b''.join(pts)] * n_rows, [b32(r) for r in rows], g2=g2)
    return out, st


@pytest.mark.parametrize('n_pts,n_rows,g2', [(37, 5, False), (37, 1, False), (1, 6, False), (9, 4, True)])
def test_rows(eng, oracle, pool, n_pts, n_rows, g2):
    rows_case(eng, oracle, pool, n_pts, n_rows, g2, 90 + n_pts + n_rows)


def test_rows_zero_row_and_forced_paths(eng, oracle, pool):
    rnd = random.Random(10)
    a, pts = draw(pool, False, 12, rnd)
    rows = [[rnd.randrange(0, 1 << 256) for _ in range(12)], [0] * 12, [R_ORDER] * 12, [rnd.randrange(0, 1 << 256) for _ in range(12)]]
    want = [want_of(oracle, a, pts, r, False) for r in rows]
    for kw in ({}, {'window': 12}, {'big': 8}, {'window': 6, 'slab': 1}):
        eng.set_msm_batch(window=0, big=0, slab=0)
        eng.set_msm_batch(**kw)
        out, st = eng.msm_rows(b''.join(pts), [b32(r) for r in rows])
        assert list(zip(out, st)) == want, kw
    assert [w[1] for w in want] == [0, 1, 1, 0]


def test_medium(eng, oracle, pool):
    """256 groups of 256 points drawn from the 64 base points: one oracle multiplication per group, and msm alone on every group"""
    rnd = random.Random(11)
    groups = []
    for g in range(256):
        a, pts = draw(pool, False, 256, rnd)
        groups.append((a, pts, [rnd.randrange(0, 1 << 256) for _ in range(256)]))
    out, st = check_batch(eng, oracle, groups)
    assert st == [0] * 256 and len(set(out)) == 256


def test_kernel_names(eng):
    assert eng.extra_program_kernel('dbladd_g1') == 'nbls_aot_dbladd_g1' and eng.extra_program_kernel('dbladd_g2') == 'nbls_aot_dbladd_g2'
    assert eng.lib.nbls_extra_program_kernel(eng.h, b'dbladd_g1').startswith(b'nbls_aot_')


def test_einval_before_any_device_work(eng, pool):
    lib, h = eng.lib, eng.h
    a, pts = pool[False]
    P, K = b''.join(pts[:4]), bytes(32 * 4)
    Q = b''.join(pool[True][1][:4])
    out, st = C.create_string_buffer(192 * 4), C.create_string_buffer(4)
    offs = (C.c_uint32 * 3)(0, 2, 4)
    assert lib.nbls_g1_msm_batch(h, 2, offs, P, K, out, st) == 0 and lib.nbls_g1_msm_rows(h, 2, P, 2, K, out, st) == 0      # the well-formed calls the others are mutations of
    assert lib.nbls_g2_msm_batch(h, 2, offs, Q, K, out, st) == 0 and lib.nbls_g2_msm_rows(h, 2, Q, 2, K, out, st) == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    too_many = (C.c_uint32 * 2)(0, (1 << 22) + 1)
    for _ in range(5):
        for f, pp in ((lib.nbls_g1_msm_batch, P), (lib.nbls_g2_msm_batch, Q)):
            assert f(None, 2, offs, pp, K, out, st) == EINVAL                                   # missing pointers
            assert f(h, 2, None, pp, K, out, st) == EINVAL
            assert f(h, 2, offs, None, K, out, st) == EINVAL
            assert f(h, 2, offs, pp, None, out, st) == EINVAL
            assert f(h, 2, offs, pp, K, None, st) == EINVAL
            assert f(h, 0, offs, pp, K, out, st) == EINVAL                                      # no group
            assert f(h, 2, (C.c_uint32 * 3)(0, 3, 2), pp, K, out, st) == EINVAL                 # decreasing offsets
            assert f(h, 2, (C.c_uint32 * 3)(3, 2, 4), pp, K, out, st) == EINVAL
            assert f(h, 1, too_many, pp, K, out, st) == EINVAL                                  # more than 2^22 points
            assert f(h, (1 << 20) + 1, offs, pp, K, out, st) == EINVAL                          # more than 2^20 groups
        for f, pp in ((lib.nbls_g1_msm_rows, P), (lib.nbls_g2_msm_rows, Q)):
            assert f(None, 2, pp, 2, K, out, st) == EINVAL
            assert f(h, 2, None, 2, K, out, st) == EINVAL
            assert f(h, 2, pp, 2, None, out, st) == EINVAL
            assert f(h, 2, pp, 2, K, None, st) == EINVAL
            assert f(h, 2, pp, 0, K, out, st) == EINVAL                                         # no row
            assert f(h, 0, pp, 2, K, out, st) == EINVAL                                         # no point: refused (documented in nbls.h)
            assert f(h, 0, pp, 0, K, out, st) == EINVAL
            assert f(h, (1 << 22) + 1, pp, 1, K, out, st) == EINVAL                             # more than 2^22 points
            assert f(h, 1 << 11, pp, (1 << 11) + 1, K, out, st) == EINVAL                       # more than 2^22 scalars
            assert f(h, 1, pp, (1 << 20) + 1, K, out, st) == EINVAL                             # more than 2^20 rows
    assert eng.lib.nbls_set_tuning(h, 16, 5) == EINVAL and eng.lib.nbls_set_tuning(h, 16, -4) == EINVAL and eng.lib.nbls_set_tuning(h, 17, -1) == EINVAL
    assert eng.lib.nbls_set_tuning(h, 18, -1) == EINVAL
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0      # 100 refused calls allocated nothing
    # and the engine is as it was
    assert lib.nbls_g1_msm_batch(h, 2, offs, P, K, out, st) == 0 and list(st.raw[:2]) == [1, 1]
