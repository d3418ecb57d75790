"""Chosen uniform bytes for everything behind expand_message_xmd in hash-to-curve: the 64-byte -> Fp reduction, both SWU maps, the addition on the isogenous curve, the isogenies
and cofactor clearing.  A SHA-256 output never lands on the inputs where these stages branch, so the lists here are built from Python integers: the representatives of the
reduction's edges, the field elements with an exceptional denominator, the t of the norm-method square root with a1 = 0 (delta = 0 among them, and roots with a zero coordinate),
seeded ordinary elements whose candidate classes are COUNTED (tests/test_oracle.py asserts the coverage this module claims), and the degenerate hash items u0 = +-u1.

Shared by tools/gen_golden.py (which hands the lists to the reference: tests/golden/ref_h2c_map.json.gz), the oracle and simulator tests and tests/test_gpu_h2c_map.py.
kind: 0 = G2 hash (256 bytes: u0.c0 u0.c1 u1.c0 u1.c1), 1 = G2 encode (128: c0 c1), 2 = G1 hash (128: u0 u1), 3 = G1 encode (64).  Everything is deterministic and built once."""
import collections
import functools
import hashlib

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
IN_BYTES = {0: 256, 1: 128, 2: 128, 3: 64}
OUT_BYTES = {0: 192, 1: 192, 2: 96, 3: 96}

Case = collections.namedtuple('Case', 'name kind uniform degenerate')


# ---- Fp and Fp2 on Python integers ----------------------------------------------------------------------------------------------------------------
def inv(x):
    return pow(x, P - 2, P)


def fsqrt(x):
    """a square root of x in Fp, or None (p = 3 mod 4)"""
    x %= P
    r = pow(x, (P + 1) // 4, P)
    return r if r * r % P == x else None


def mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def conj(a):
    return (a[0], (-a[1]) % P)


def norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def inv2(a):
    n = inv(norm(a))
    return (a[0] * n % P, (-a[1]) * n % P)


def pow2(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = mul(r, r)
        if bit == '1':
            r = mul(r, a)
    return r


def sqrt2(a):
    """a square root of a in Fp2 = Fp[i], or None: the real part x0 of a root has x0^2 = (a0 +- sqrt(N(a))) / 2"""
    a = (a[0] % P, a[1] % P)
    if a == (0, 0):
        return (0, 0)
    n = fsqrt(norm(a))
    if n is None:
        return None
    for s in (n, -n):
        x0 = fsqrt((a[0] + s) * inv(2))
        if x0:
            r = (x0, a[1] * inv(2 * x0) % P)
            if mul(r, r) == a:
                return r
    h = fsqrt(-a[0])            # a purely imaginary root
    if h is not None and mul((0, h), (0, h)) == a:
        return (0, h)
    return None


def quadratic2(b, c):
    """the roots of s^2 + b s + c over Fp2"""
    d = sqrt2(sub(mul(b, b), mul((4, 0), c)))
    if d is None:
        return []
    h = (inv(2), 0)
    return [mul(sub(d, b), h), mul(sub(neg(d), b), h)]


# ---- the SWU maps as the algorithms state them (draft-irtf-cfrg-hash-to-curve, appendix G.2): only what the case lists and their coverage test need ---------------------
Z2, A2, B2, ONE = ((-2) % P, (-1) % P), (0, 240), (1012, 1012), (1, 0)
XI = (1, 1)
ROOTS8 = [pow2(XI, (P * P - 1) * k // 8) for k in range(4)]          # the four "positive" eighth roots of unity: 1, i, sqrt(i), sqrt(-i)
SQRT_M125 = fsqrt(-125)


def _etas():
    """eta_k with eta_k^2 = Z^3 zeta for the four primitive eighth roots of unity zeta (the order is immaterial here: only WHICH candidate fits is classified)"""
    z3 = mul(mul(Z2, Z2), Z2)
    out = []
    for k in (1, 3, 5, 7):
        e = sqrt2(mul(z3, pow2(XI, (P * P - 1) * k // 8)))
        assert e is not None
        out.append(e)
    return out


ETAS = _etas()


def swu2_prepare(t):
    zt2 = mul(Z2, mul(t, t))
    ztzt = add(zt2, mul(zt2, zt2))
    den = neg(mul(A2, ztzt))
    num = mul(B2, add(ztzt, ONE))
    exceptional = den == (0, 0)
    if exceptional:
        den = mul(Z2, A2)
    v = mul(mul(den, den), den)
    u = add(add(mul(mul(num, num), num), mul(mul(A2, num), mul(den, den))), mul(B2, v))
    return zt2, num, den, u, v, exceptional


def sgn0_2(x):
    return bool(x[0] % 2 or (x[0] == 0 and x[1] % 2))


def swu2_classes(t):
    """what the two square-root methods meet at t: success (g(x0) is a square), the root of unity res / gamma (index 0..3, None without success), the eta candidate (index of the
    class of ec / x1c, None with success), and for the norm method a1 == 0, delta == 0, pos, and whether the root it forms has a zero coordinate; plus the map's output (x, y)"""
    zt2, num, den, u, v, exceptional = swu2_prepare(t)
    v7 = pow2(v, 7)
    uv7 = mul(u, v7)
    uv15 = mul(uv7, mul(v7, v))
    gamma = mul(pow2(uv15, (P * P - 9) // 16), uv7)
    root = next((k for k in range(4) if mul(mul(mul(ROOTS8[k], gamma), mul(ROOTS8[k], gamma)), v) == u), None)
    success = root is not None
    zt2_3 = mul(mul(zt2, zt2), zt2)
    u2 = mul(zt2_3, u)
    eta = None
    if success:
        y = mul(ROOTS8[root], gamma)
    else:
        x1c = mul(gamma, mul(mul(t, t), t))
        # the class of the fitting candidate: eta_k^2 runs through Z^3 zeta, so exactly one k has (eta_k x1c)^2 v = u2 up to the sign of eta_k
        eta = next(k for k in range(4) if mul(mul(mul(ETAS[k], x1c), mul(ETAS[k], x1c)), v) == u2)
        y = mul(ETAS[eta], x1c)
        num = mul(num, zt2)
    if sgn0_2(t) != sgn0_2(y):
        y = neg(y)
    x = mul(num, inv2(den))
    # the norm method (csrc/codec.h swu_norm_*)
    a = mul(u, conj(v))
    d = norm(v)
    n = pow(norm(a), (P + 1) // 4, P)
    assert (n * n % P == norm(a)) == success
    as_, ns = (a, n) if success else (mul(a, zt2_3), n * SQRT_M125 % P * pow(norm(t), 3, P) % P)
    half = inv(2)
    d0 = (as_[0] + ns) * half % P
    delta = as_[0] if d0 == 0 else d0
    g = delta * pow(d, 3, P) % P
    e = pow(g, (P - 3) // 4, P)
    q = d * e % P
    r = delta * q % P
    other = as_[1] * half % P * (r * q * q % P * d % P) % P
    pos = (r * r % P * d - delta) % P == 0
    yn = (r, other) if pos else (other, r)
    assert mul(mul(yn, yn), v) == (u if success else u2), 'the norm method misses its root'
    return {'success': success, 'root': root, 'eta': eta, 'exceptional': exceptional, 'a1_zero': as_[1] == 0, 'delta_zero': d0 == 0, 'pos': pos,
            'zero_coord': yn[0] == 0 or yn[1] == 0, 'x': x, 'y': y}


G1_A = 0x144698a3b8e9433d693a02c96d4982b0ea985383ee66a8d8e8981aefd881ac98936f8da0e0f97f5cf428082d584c1d
G1_B = 0x12e2908d11688030018b12e8753eee3b2016c1f0f24f4070a0b9c14fcef35ef55a23215a316ceaa5d1cc48e98e172be0
G1_Z = 11


def swu1_classes(u):
    """G1 map: the exceptional denominator and the outcome of y1^2 gxd == gx1"""
    tv3 = G1_Z * u * u % P
    xd0 = (tv3 * tv3 + tv3) % P
    xn1 = (xd0 + 1) * G1_B % P
    xd = (-G1_A) * xd0 % P
    exceptional = xd == 0
    if exceptional:
        xd = G1_A * G1_Z % P
    gxd = pow(xd, 3, P)
    gx1 = (pow(xn1, 3, P) + G1_A * xn1 % P * xd * xd + G1_B * gxd) % P
    tv2 = gx1 * gxd % P
    y1 = pow(gxd * gxd % P * tv2 % P, (P - 3) // 4, P) * tv2 % P
    return {'exceptional': exceptional, 'first': y1 * y1 % P * gxd % P == gx1}


# ---- the elements ----------------------------------------------------------------------------------------------------------------------------------
def be64(v):
    assert 0 <= v < 1 << 512
    return v.to_bytes(64, 'big')


def _seeded(tag, k):
    """64 bytes from SHA-256 of a counter"""
    return hashlib.sha256(b'nbls-h2c-cases:%s:%d:0' % (tag, k)).digest() + hashlib.sha256(b'nbls-h2c-cases:%s:%d:1' % (tag, k)).digest()


K_TOP = ((1 << 512) - 1) // P                     # the largest K with K p < 2^512
# 64-byte strings (as integers) at the edges of os2ip(64 bytes) mod p = top16 * 2^384 + low48: zero, all ones, next to p and to its multiples, next to 2^384 (the first
# value with a top part), the top bit alone, and each part saturated with the other one empty (top16 = 0 with low48 = ff..ff is 2^384 - 1)
REPRESENTATIVES = [('0', 0), ('2^512-1', (1 << 512) - 1), ('p-1', P - 1), ('p', P), ('p+1', P + 1), ('2p', 2 * P), ('2^384-1', (1 << 384) - 1), ('2^384', 1 << 384),
                   ('2^384+1', (1 << 384) + 1), ('Kp-1', K_TOP * P - 1), ('Kp', K_TOP * P), ('Kp+1', K_TOP * P + 1), ('2^511', 1 << 511),
                   ('top16=ff..ff,low48=0', ((1 << 128) - 1) << 384)]
assert K_TOP * P < 1 << 512 <= (K_TOP + 1) * P

ORD_FP = int.from_bytes(_seeded(b'fixed', 0), 'big') % P                                  # the one fixed ordinary element of the slots not under test
ORD_FP2 = (ORD_FP, int.from_bytes(_seeded(b'fixed', 1), 'big') % P)

G2_STRUCTURED = [('(0,0)', (0, 0)), ('(0,1)', (0, 1)), ('(0,2)', (0, 2)), ('(0,p-1)', (0, P - 1)), ('(1,0)', (1, 0)), ('(2,0)', (2, 0)), ('(p-1,0)', (P - 1, 0))]
SQRT_M1_11 = fsqrt(-inv(11))                      # 11 u^2 = -1: the non-zero u with an exceptional denominator in G1
assert SQRT_M1_11 is not None
G1_STRUCTURED = [('0', 0), ('+sqrt(-1/11)', SQRT_M1_11), ('-sqrt(-1/11)', P - SQRT_M1_11), ('1', 1), ('2', 2), ('p-1', P - 1), ('p-2', P - 2)]


def _real_g(leg, imag_bound=64):
    """t whose norm-method operand has a1 = 0.  The operand is g(x) N(v) with g(x) = x^3 + 240 i x + 1012 (1 + i) and x = x0(t) when g(x0) is a square (leg 1), x = x1(t) =
    Z t^2 x0(t) when it is not (leg 2), so a1 = 0 means g(x) in Fp.  For x = a + b i that is 3 a^2 b - b^3 + 240 a + 1012 = 0: a quadratic in a for each small b.  From x back
    to s = Z t^2 with w = s + s^2:  x0 = -B/A (1 + 1/w), x1 = -B/A (s + 1/(1 + s)), each a quadratic in s; then t = sqrt(s / Z), and -t."""
    found = []
    for b in range(imag_bound):
        if b == 0:
            real = [(-1012) * inv(240) % P]
        else:
            s = fsqrt(240 * 240 - 12 * b * (1012 - b ** 3))
            if s is None:
                continue
            real = [(-240 + s) * inv(6 * b) % P, (-240 - s) * inv(6 * b) % P]
        for a in real:
            x = (a, b)
            q = neg(mul(mul(x, A2), inv2(B2)))                                # x = -B/A q
            if leg == 1:
                q1 = sub(q, ONE)
                if q1 == (0, 0):
                    continue
                roots = quadratic2(ONE, neg(inv2(q1)))                         # s^2 + s - 1/(q - 1) = 0
            else:
                roots = quadratic2(sub(ONE, q), sub(ONE, q))                   # s^2 + (1 - q) s + (1 - q) = 0
            for s2 in roots:
                t = sqrt2(mul(s2, inv2(Z2)))
                if t is None or t == (0, 0):
                    continue
                for tt in (t, neg(t)):
                    c = swu2_classes(tt)
                    if c['success'] == (leg == 1) and c['a1_zero']:
                        found.append((b, tt, c))
    return found


@functools.lru_cache(maxsize=None)
def a1_zero_family():
    """(name, t) of the a1 = 0 family of leg 1 (x0 real-valued g) and of leg 2: every t found for Im x < 64 whose class -- (leg, delta = 0, pos, root with a zero coordinate,
    sgn0 t) -- has not been seen twice already, so that the list stays short while every class the search reaches is kept, each with both a t and its -t"""
    out, seen = [], collections.Counter()
    for leg in (1, 2):
        for b, t, c in _real_g(leg):
            key = (leg, c['delta_zero'], c['pos'], c['zero_coord'], sgn0_2(t))
            if seen[key] >= 2:
                continue
            seen[key] += 1
            out.append(('a1=0 leg%d Im x=%d delta%s0 pos=%d sgn0=%d #%d' % (leg, b, '=' if c['delta_zero'] else '!=', c['pos'], sgn0_2(t), seen[key]), t))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g2_elements():
    """every G2 field element under test as (name, c0 string, c1 string), the strings as integers below 2^512"""
    els = [('c0=' + n, v, ORD_FP2[1]) for n, v in REPRESENTATIVES] + [('c1=' + n, ORD_FP2[0], v) for n, v in REPRESENTATIVES]
    els += [('t=' + n, t[0], t[1]) for n, t in G2_STRUCTURED]
    els += [(n, t[0], t[1]) for n, t in a1_zero_family()]
    return tuple(els)


@functools.lru_cache(maxsize=None)
def g2_seeded():
    return tuple(('seeded %d' % k, int.from_bytes(_seeded(b'g2c0', k), 'big'), int.from_bytes(_seeded(b'g2c1', k), 'big')) for k in range(64))


@functools.lru_cache(maxsize=None)
def g1_elements():
    """(name, 64-byte string as an integer): the representatives, then the structured elements they do not already hold (0 and p - 1 are in both lists)"""
    return tuple(('u=' + n, v) for n, v in REPRESENTATIVES + [e for e in G1_STRUCTURED if e not in REPRESENTATIVES])


@functools.lru_cache(maxsize=None)
def g1_seeded():
    return tuple(('seeded %d' % k, int.from_bytes(_seeded(b'g1', k), 'big')) for k in range(32))


# ---- the case lists --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(kind):
    """the case list of one kind, degenerate items last"""
    out = []
    if kind in (0, 1):
        ordinary = be64(ORD_FP2[0]) + be64(ORD_FP2[1])
        el, sd = [(n, be64(c0) + be64(c1)) for n, c0, c1 in g2_elements()], [(n, be64(c0) + be64(c1)) for n, c0, c1 in g2_seeded()]
    else:
        ordinary = be64(ORD_FP)
        el, sd = [(n, be64(v)) for n, v in g1_elements()], [(n, be64(v)) for n, v in g1_seeded()]
    if kind in (1, 3):
        out = [Case(n, kind, b, False) for n, b in el + sd]
    else:
        out = [Case('u0: ' + n, kind, b + ordinary, False) for n, b in el] + [Case('u1: ' + n, kind, ordinary + b, False) for n, b in el]
        out += [Case('%s | %s' % (sd[k][0], sd[k + 1][0]), kind, sd[k][1] + sd[k + 1][1], False) for k in range(0, len(sd), 2)]
        # u0 = +-u1 mod p: the two SWU points are equal or opposite, where the reference's addition doubles or returns zero (and throws on the way to affine)
        if kind == 0:
            minus, plus_p = be64(P - ORD_FP2[0]) + be64(P - ORD_FP2[1]), be64(ORD_FP2[0] + P) + be64(ORD_FP2[1] + P)
        else:
            minus, plus_p = be64(P - ORD_FP), be64(ORD_FP + P)
        out += [Case('degenerate (u0, u0)', kind, ordinary + ordinary, True), Case('degenerate (u0, -u0)', kind, ordinary + minus, True),
                Case('degenerate (u0, u0 + p)', kind, ordinary + plus_p, True)]
    assert all(len(c.uniform) == IN_BYTES[kind] for c in out) and len({c.name for c in out}) == len(out)
    return tuple(out)


def elements_of(case):
    """the field elements of a case as reduced integers: Fp2 pairs for kinds 0 and 1, Fp values for 2 and 3"""
    v = [int.from_bytes(case.uniform[k:k + 64], 'big') % P for k in range(0, len(case.uniform), 64)]
    return [(v[k], v[k + 1]) for k in range(0, len(v), 2)] if case.kind in (0, 1) else v
