"""Known-answer tests of the single tower operations on the device (nbls_tower_op_batch, include/nbls.h): the vectors tools/gen_golden.mjs produced by running the
reference itself (Fp / Fp2 / Fp6 / Fp12 add, subtract, multiply, square, invert, Frobenius maps, conjugate, multiplication by the non-residue, the sparse products
multiplyBy1 / 01 / 014, cyclotomicSquare, cyclotomicExp: math.ts:223-273, 451-539, 601-688, 732-852), plus algebraic identities where the file holds no vector
(Frobenius powers composed from the first one, a * a^-1 = 1, unitary inverse = conjugate).  Square roots are covered through the decoders (tests/test_gpu_codec.py).
Then every operation of every field with BOTH operands extremal (tests/field_cases.py: the ends of the range, saturated and alternating limbs, sparse elements), at batch sizes
that end inside and on a wavefront, against Python integers (Fp, Fp2, the coefficient-wise operations) and the oracle (Fp6, Fp12)."""
import importlib
import pytest
from field_cases import tower_elements
from goldenio import hx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)

ADD, SUB, NEG, MUL, SQR, INV, FROB, CONJ, MULNR, MULB, MUL1, MUL01, MUL014, CYCSQR, CYCEXP = range(15)
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def cat(vs, key):
    return b''.join(hx(v[key]) for v in vs)


def test_fp_ops(engine, golden):
    vs = [v for v in golden['fp'] if v['inv'] is not None]
    a, b = cat(vs, 'a'), cat(vs, 'b')
    for op, key in ((ADD, 'add'), (SUB, 'sub'), (MUL, 'mul')):
        assert engine.tower_op(1, op, a, b) == cat(vs, key), key
    for op, key in ((NEG, 'neg'), (SQR, 'sqr'), (INV, 'inv')):
        assert engine.tower_op(1, op, a) == cat(vs, key), key
    # the zero element and p - 1: negate / square / multiply at the edges of the range
    edge = (0).to_bytes(48, 'big') + (P - 1).to_bytes(48, 'big') + (1).to_bytes(48, 'big')
    assert engine.tower_op(1, NEG, edge) == (0).to_bytes(48, 'big') + (1).to_bytes(48, 'big') + (P - 1).to_bytes(48, 'big')
    assert engine.tower_op(1, SQR, edge) == (0).to_bytes(48, 'big') + (1).to_bytes(48, 'big') + (1).to_bytes(48, 'big')
    assert engine.tower_op(1, INV, edge[48:]) == (P - 1).to_bytes(48, 'big') + (1).to_bytes(48, 'big')


def test_fp2_ops(engine, golden):
    vs = golden['fp2']
    a, b = cat(vs, 'a'), cat(vs, 'b')
    for op, key in ((ADD, 'add'), (SUB, 'sub'), (MUL, 'mul')):
        assert engine.tower_op(2, op, a, b) == cat(vs, key), key
    for op, key in ((SQR, 'sqr'), (INV, 'inv'), (MULNR, 'mulnr'), (MULB, 'mulB')):
        assert engine.tower_op(2, op, a) == cat(vs, key), key
    assert engine.tower_op(2, FROB, a, param=1) == cat(vs, 'frob1')
    assert engine.tower_op(2, CONJ, a) == cat(vs, 'frob1')
    assert engine.tower_op(2, FROB, a, param=2) == a


def test_fp6_ops(engine, golden):
    vs = golden['fp6']
    a, b = cat(vs, 'a'), cat(vs, 'b')
    assert engine.tower_op(6, MUL, a, b) == cat(vs, 'mul')
    for op, key in ((SQR, 'sqr'), (INV, 'inv'), (MULNR, 'mulnr')):
        assert engine.tower_op(6, op, a) == cat(vs, key), key
    assert engine.tower_op(6, MUL1, a, cat(vs, 'b1')) == cat(vs, 'mul1')
    assert engine.tower_op(6, MUL01, a, cat(vs, 'b0'), cat(vs, 'b1')) == cat(vs, 'mul01')
    for k in range(1, 6):
        assert engine.tower_op(6, FROB, a, param=k) == b''.join(hx(v['frob'][k - 1]) for v in vs), k
    assert engine.tower_op(6, FROB, a, param=6) == a
    # a * a^-1 = 1
    one = (1).to_bytes(48, 'big') + bytes(5 * 48)
    assert engine.tower_op(6, MUL, a, cat(vs, 'inv')) == one * len(vs)


def test_fp12_ops(engine, golden):
    vs = golden['fp12']
    a, b = cat(vs, 'a'), cat(vs, 'b')
    assert engine.tower_op(12, MUL, a, b) == cat(vs, 'mul')
    for op, key in ((SQR, 'sqr'), (INV, 'inv'), (CONJ, 'conj')):
        assert engine.tower_op(12, op, a) == cat(vs, key), key
    assert engine.tower_op(12, MUL014, a, cat(vs, 'o0'), cat(vs, 'o1'), cat(vs, 'o4')) == cat(vs, 'mul014')
    for i, k in enumerate((1, 2, 3, 6)):
        assert engine.tower_op(12, FROB, a, param=k) == b''.join(hx(v['frob'][i]) for v in vs), k
    # Frobenius maps the golden file does not hold: phi^k composed from phi^1, and phi^12 = identity
    x = a
    for k in range(1, 13):
        x = engine.tower_op(12, FROB, x, param=1)
        if k < 12:
            assert engine.tower_op(12, FROB, a, param=k) == x, k
    assert x == a
    u = cat(vs, 'unitary')
    assert engine.tower_op(12, CYCSQR, u) == cat(vs, 'cyclosqr')
    assert engine.tower_op(12, CYCEXP, u) == cat(vs, 'cycloexp')
    # on unitary elements the cyclotomic square is the square and the inverse is the conjugate
    assert engine.tower_op(12, SQR, u) == cat(vs, 'cyclosqr')
    assert engine.tower_op(12, INV, u) == engine.tower_op(12, CONJ, u)
    # a non-unitary inverse: a * a^-1 = 1
    one = (1).to_bytes(48, 'big') + bytes(11 * 48)
    assert engine.tower_op(12, MUL, a, cat(vs, 'inv')) == one * len(vs)


def test_unsupported_combinations_are_rejected(engine, golden):
    import importlib
    pkg = importlib.import_module('noble-bls12-381_amd')
    a = cat(golden['fp6'], 'a')
    for field, op in ((6, CONJ), (1, FROB), (2, MUL014), (12, MULB), (7, ADD)):
        with pytest.raises(pkg.NblsError):
            engine.tower_op(field, op, a[:48 * field] if field != 7 else a[:48])


# ---- extremal operands in both places, batches that end inside a wavefront
BATCHES = (1, 7, 63, 64, 65, 129, 300)
N_CASES = max(BATCHES)
FNAME = {1: 'Fp', 2: 'Fp2', 6: 'Fp6', 12: 'Fp12'}
UNARY = {NEG: 'neg', SQR: 'sqr', INV: 'inv', CONJ: 'conj', MULNR: 'mulnr', MULB: 'mulB'}
BINARY = {ADD: 'add', SUB: 'sub', MUL: 'mul'}


def _ops():
    """(field, op, param, name) of everything nbls_tower_op_batch accepts"""
    out = []
    for field, ops in ((1, (ADD, SUB, NEG, MUL, SQR, INV)), (2, (ADD, SUB, NEG, MUL, SQR, INV, CONJ, MULNR, MULB)), (6, (ADD, SUB, NEG, MUL, SQR, INV, MULNR)),
                       (12, (ADD, SUB, NEG, MUL, SQR, INV, CONJ))):
        out += [(field, op, 0, {**UNARY, **BINARY}[op]) for op in ops]
        if field != 1:
            out += [(field, FROB, k, 'frob%d' % k) for k in range(12)]
    out += [(6, MUL1, 0, 'mulBy1'), (6, MUL01, 0, 'mulBy01'), (12, MUL014, 0, 'mulBy014'), (12, CYCSQR, 0, 'cyclotomicSquare'), (12, CYCEXP, 0, 'cyclotomicExp')]
    return out


def _enc(coefs):
    return b''.join(v.to_bytes(48, 'big') for v in coefs)


def _dec(b):
    return [int.from_bytes(b[i:i + 48], 'big') for i in range(0, len(b), 48)]


def _f2mul(a, b):
    return [(a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P]


def _python_reference(field, op, param, a, b):
    """Fp and Fp2 on Python integers (math.ts:223-273, 451-539); the coefficient-wise operations of every field"""
    if op == ADD: return [(x + y) % P for x, y in zip(a, b)]
    if op == SUB: return [(x - y) % P for x, y in zip(a, b)]
    if op == NEG: return [(-x) % P for x in a]
    if field == 1:
        return [{MUL: lambda: a[0] * b[0], SQR: lambda: a[0] * a[0], INV: lambda: pow(a[0], -1, P)}[op]() % P]
    assert field == 2
    if op == MUL: return _f2mul(a, b)
    if op == SQR: return _f2mul(a, a)
    if op == INV:
        ni = pow(a[0] * a[0] + a[1] * a[1], -1, P)
        return [a[0] * ni % P, -a[1] * ni % P]
    if op == CONJ or op == FROB: return [a[0], -a[1] % P] if (op == CONJ or param % 2) else list(a)
    if op == MULNR: return [(a[0] - a[1]) % P, (a[0] + a[1]) % P]
    if op == MULB: return [4 * (a[0] - a[1]) % P, 4 * (a[0] + a[1]) % P]
    raise AssertionError(op)


def _reference(oracle, field, op, param, a, b, c, d):
    if field <= 2 or op in (ADD, SUB, NEG):
        return _enc(_python_reference(field, op, param, _dec(a), _dec(b) if b else None))
    esz, f = 48 * field, 'fp%d_' % field
    if op == MUL: return oracle.bin(f + 'mul', a, b, esz)
    if op in (SQR, INV): return oracle.un(f + UNARY[op], a, esz)
    if op == FROB: return (oracle.fp6_frob if field == 6 else oracle.fp12_frob)(a, param)
    if op == MULNR: return oracle.un('fp6_mulnr', a, esz)
    if op == CONJ: return oracle.un('fp12_conj', a, esz)
    if op == MUL1: return oracle.call('fp6_mul_by_1', esz, a, b)[1]
    if op == MUL01: return oracle.call('fp6_mul_by_01', esz, a, b, c)[1]
    if op == MUL014: return oracle.call('fp12_mul_by_014', esz, a, b, c, d)[1]
    if op == CYCSQR: return oracle.un('fp12_cyclotomic_sqr', a, esz)
    if op == CYCEXP: return oracle.un('fp12_cyclotomic_exp_x', a, esz)
    raise AssertionError(op)


def _build_pools(oracle):
    """per field: the extremal elements as wire bytes, the zero element last; 'unitary': frob2(u) u with u = conj(f) / f of every non-zero extremal Fp12 element f"""
    pools = {field: [_enc(c) for c in tower_elements(field)] for field in (1, 2, 6, 12)}
    for field, pool in pools.items():
        assert pool[-1] == bytes(48 * field) and all(any(e) for e in pool[:-1])
    uni = []
    for f in pools[12][:-1]:
        u = oracle.bin('fp12_mul', oracle.un('fp12_conj', f, 576), oracle.un('fp12_inv', f, 576), 576)
        uni.append(oracle.bin('fp12_mul', oracle.fp12_frob(u, 2), u, 576))
    pools['unitary'] = uni
    return pools


@pytest.fixture(scope='module')
def pools(oracle):
    return _build_pools(oracle)


def _operands(pools, field, op):
    """N_CASES operand tuples (a, b, c, d), both operands walking the pool at different strides (Fp: every ordered pair of extremes); b / c / d of the sparse products are Fp2
    elements.  Inversion leaves out the zero element -- its output is unspecified -- and nothing else; the cyclotomic operations take the unitary elements."""
    A = pools['unitary'] if op in (CYCSQR, CYCEXP) else pools[field][:-1] if op == INV else pools[field]
    Bp = pools[2] if op in (MUL1, MUL01, MUL014) else pools[field]
    L, L2 = len(A), len(Bp)
    cases = []
    for i in range(N_CASES):
        q = i // L
        a = A[i % L]
        b = Bp[(i % L + 1 + 17 * q) % L2] if (op in BINARY or op in (MUL1, MUL01, MUL014)) else None
        c = pools[2][(3 * i + 1 + q) % len(pools[2])] if op in (MUL01, MUL014) else None
        d = pools[2][(5 * i + 2 + 3 * q) % len(pools[2])] if op == MUL014 else None
        cases.append((a, b, c, d))
    return cases


def test_every_ordered_pair_of_fp_extremes_is_a_case(pools):
    cases = _operands(pools, 1, MUL)
    assert {(a, b) for a, b, _, _ in cases} == {(a, b) for a in pools[1] for b in pools[1]}
    assert bytes(48) not in [a for a, _, _, _ in _operands(pools, 1, INV)] and len({a for a, _, _, _ in _operands(pools, 1, INV)}) == len(pools[1]) - 1


@pytest.mark.parametrize('field,op,param,name', [pytest.param(*o, id='%s-%s' % (FNAME[o[0]], o[3])) for o in _ops()])
def test_extremal_operands_and_wavefront_edges(engine, oracle, pools, field, op, param, name):
    """one operation on operands that are extremal in BOTH places, cycled through batches of 1, 7, 63, 64, 65, 129 and 300 items; every item compared on its own"""
    esz = 48 * field
    cases = _operands(pools, field, op)
    want = [_reference(oracle, field, op, param, *c) for c in cases]
    for n in BATCHES:
        cols = [b''.join(c[j] for c in cases[:n]) if cases[0][j] is not None else None for j in range(4)]
        out = engine.tower_op(field, op, cols[0], cols[1], cols[2], cols[3], param=param)
        assert len(out) == esz * n
        for i in range(n):
            assert out[esz * i:esz * i + esz] == want[i], 'field %s op %s n %d index %d: a = %s' % (FNAME[field], name, n, i, cases[i][0].hex())
