"""The scalar field Fr and the Lagrange coefficients at zero without a GPU: fr_exec.h -- the file fr_kernels.hip compiles for the device -- on the simulator (nbls_sim_fr_*)
against the reference's own Fr vectors (tests/golden/ref_fr.json.gz, tools/gen_golden_fr.mjs) and against Python integers.  Everything is bit-exact."""
import ctypes as C
import random
import pytest
import goldenio
import vmsim_py

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # CURVE.r (reference math.ts:15)
M256 = (1 << 256) - 1
OPS = {'add': 0, 'sub': 1, 'neg': 2, 'mul': 3, 'sqr': 4, 'inv': 5, 'div': 6, 'pow': 7}
UNARY = ('neg', 'sqr', 'inv')
EDGES = [0, 1, R - 1, R, R + 1, M256]
BAD_IDS = 20


@pytest.fixture(scope='module')
def sim():
    return vmsim_py.load()


@pytest.fixture(scope='module')
def fr_golden():
    return goldenio.load('ref_fr.json.gz')


def b32(v):
    return v.to_bytes(32, 'big')


def fr_op(sim, op, a, b=None):
    n = len(a)
    out, st = C.create_string_buffer(32 * n), C.create_string_buffer(n)
    sim.nbls_sim_fr_op(C.c_uint(n), OPS[op], b''.join(map(b32, a)), None if b is None else b''.join(map(b32, b)), out, st)
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], 'big') for i in range(n)], list(st.raw)


def py_op(op, a, b):
    """-> (value, status) as nbls_fr_op_batch defines them"""
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
    """-> the coefficients, or None for unusable identifiers"""
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


def lagrange(sim, groups):
    sizes = [len(g) for g in groups]
    offs = [0]
    for t in sizes:
        offs.append(offs[-1] + t)
    n = offs[-1]
    out, st = C.create_string_buffer(32 * n), C.create_string_buffer(len(groups))
    sim.nbls_sim_fr_lagrange(C.c_uint(n), C.c_uint(len(groups)), (C.c_uint32 * len(offs))(*offs), b''.join(b32(x) for g in groups for x in g), out, st)
    vals = [int.from_bytes(out.raw[32 * k:32 * k + 32], 'big') for k in range(n)]
    return [vals[offs[g]:offs[g + 1]] for g in range(len(groups))], list(st.raw)


def check_groups(sim, groups):
    got, st = lagrange(sim, groups)
    for g, ids in enumerate(groups):
        want = py_lagrange(ids)
        if want is None:
            assert st[g] == BAD_IDS and got[g] == [0] * len(ids), g
        else:
            assert st[g] == 0 and got[g] == want, (g, len(ids))


def test_constants_against_python_integers(sim, fr_golden):
    w = (C.c_uint32 * 33)()
    sim.nbls_sim_fr_consts(w)
    limbs = lambda k: sum(w[k + i] << (32 * i) for i in range(8))
    assert int(fr_golden['r'], 16) == R
    assert limbs(0) == R
    assert w[8] == -pow(R, -1, 1 << 32) % (1 << 32)
    assert limbs(9) == (1 << 512) % R
    assert limbs(17) == (1 << 256) % R
    assert limbs(25) == R - 2
    assert 2 * R < 1 << 256          # what the single masked subtraction after a product relies on


def test_every_op_against_the_reference_vectors(sim, fr_golden):
    v = fr_golden['fr_ops']
    assert len(v) >= 40
    a = [int(x['a'], 16) for x in v]
    b = [int(x['b'], 16) for x in v]
    e = [int(x['e'], 16) for x in v]
    assert set(EDGES) <= set(a) and set(EDGES) <= set(b)
    for op in OPS:
        got, st = fr_op(sim, op, a, None if op in UNARY else (e if op == 'pow' else b))
        for i, x in enumerate(v):
            if x[op] is None:        # the reference throws: invert of 0
                assert st[i] == 5 and got[i] == 0, (op, i)
            else:
                assert st[i] == 0 and got[i] == int(x[op], 16), (op, i)
    assert any(x['inv'] is None for x in v) and any(x['div'] is None for x in v)


def test_every_op_against_python_integers(sim):
    rnd = random.Random(381)
    vals = EDGES + [2, R - 2, 2 * R, 2 * R + 1, M256 - 1, 1 << 255, (1 << 32) - 1, 1 << 32, (1 << 224) - 1] + [rnd.getrandbits(256) for _ in range(40)]
    a = [x for x in vals for _ in EDGES] + vals
    b = [y for _ in vals for y in EDGES] + vals[::-1]
    for op in OPS:
        got, st = fr_op(sim, op, a, None if op in UNARY else b)
        for i in range(len(a)):
            assert (got[i], st[i]) == py_op(op, a[i], b[i]), (op, hex(a[i]), hex(b[i]))
        assert all(x < R for x in got)


def test_inv_and_div_of_zero(sim):
    zeros = [0, R, 2 * R]
    got, st = fr_op(sim, 'inv', zeros)
    assert got == [0, 0, 0] and st == [5, 5, 5]
    got, st = fr_op(sim, 'div', [7, R - 1, 0], zeros)
    assert got == [0, 0, 0] and st == [5, 5, 5]
    got, st = fr_op(sim, 'div', zeros, [3, 3, 3])
    assert got == [0, 0, 0] and st == [0, 0, 0]


def test_conversion_round_trip(sim):
    rnd = random.Random(7)
    vals = EDGES + [rnd.getrandbits(256) for _ in range(20)]
    n = len(vals)
    mont, back = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    sim.nbls_sim_fr_convert(C.c_uint(n), 1, b''.join(map(b32, vals)), mont)
    for i, v in enumerate(vals):
        assert int.from_bytes(mont.raw[32 * i:32 * i + 32], 'little') == (v << 256) % R        # Montgomery form, little-endian limbs, canonical
    sim.nbls_sim_fr_convert(C.c_uint(n), 0, mont, back)
    assert [int.from_bytes(back.raw[32 * i:32 * i + 32], 'big') for i in range(n)] == [v % R for v in vals]


@pytest.mark.parametrize('t', [1, 2, 3, 7, 63, 64, 65, 667])
def test_lagrange_against_python_integers(sim, t):
    rnd = random.Random(t)
    ids = list(range(1, t + 1))
    big = [rnd.getrandbits(256) for _ in range(t)]
    over = [R + 1 + rnd.randrange(R - 2) for _ in range(t)]          # identifiers >= r
    shuffled = ids[:]
    rnd.shuffle(shuffled)
    check_groups(sim, [ids])
    check_groups(sim, [big])
    check_groups(sim, [over])
    # the same groups side by side in one call: they straddle tiles and wavefronts differently, and the small neighbours move every boundary
    check_groups(sim, [[5], ids, big, [2, 9], over, shuffled, [R - 1, 1, 2]])


def test_lagrange_many_small_groups_and_boundaries(sim):
    rnd = random.Random(3)
    check_groups(sim, [[rnd.getrandbits(256) for _ in range(3)] for _ in range(100)])
    # group sizes 1 .. 130 back to back: a boundary at every position of a wavefront
    check_groups(sim, [[rnd.getrandbits(256) for _ in range(t)] for t in range(1, 131)])
    # a group boundary exactly at lanes 63 | 64 and 127 | 128
    check_groups(sim, [list(range(1, 65)), list(range(1, 65)), [1, 2, 3]])


def test_lagrange_bad_identifiers_stay_in_their_group(sim):
    rnd = random.Random(11)
    x = rnd.getrandbits(250)
    good = [rnd.getrandbits(256) for _ in range(70)]
    groups = [good, [1, 2, x, 3, x + R],          # the colliding pair x and x + r
              [4, 5, 6], [7, R, 8],                # an identifier equal to r
              good[:5], [0], [9, 9], [3], good + [good[64]],      # duplicates across a tile boundary
              [1, 2, 3], [2 * R, 5]]
    got, st = lagrange(sim, groups)
    assert st == [0, BAD_IDS, 0, BAD_IDS, 0, BAD_IDS, BAD_IDS, 0, BAD_IDS, 0, BAD_IDS]
    check_groups(sim, groups)


def test_lagrange_matches_the_reference_cases(sim, fr_golden):
    cases = fr_golden['threshold']
    got, st = lagrange(sim, [[int(x, 16) for x in c['ids']] for c in cases])
    assert st == [0] * len(cases)
    for c, g in zip(cases, got):
        assert g == [int(x, 16) for x in c['lambda']]
