"""Operand lists shared by the host-simulator tests (tests/test_vm_sim.py) and the device tests (tests/test_gpu_field_kernels.py, test_gpu_tower.py, test_gpu_adversarial.py) of the
field arithmetic, so that the device sees exactly the structured values the host model is checked on: raw scratch elements for the stand-alone inversion and fixed-exponent
kernels, and the extremal field elements the tower operations and the pairing entry points are fed.  Every list is deterministic (seeded) and built once per process."""
import functools
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 1 << 392          # the Montgomery radix of the raw elements: 14 limbs of 28 bits
RAW = 64              # bytes of one raw element: 14 little-endian 28-bit limbs in 32-bit words, then 8 zero bytes
EXPONENTS = {0: (P + 1) // 4, 1: (P * P + 7) // 16, 2: (P * P - 9) // 16, 3: (P - 3) // 4}      # run_pow's `which` -> exponent


def raw(xs):
    """integers below 2^392 -> raw elements, limbs taken as they are (no reduction, no Montgomery factor)"""
    return b''.join(b''.join(((x >> (28 * i)) & 0xfffffff).to_bytes(4, 'little') for i in range(14)) + bytes(8) for x in xs)


def words(buf, k):
    """the sixteen 32-bit words of element k"""
    o = buf[RAW * k:RAW * k + RAW]
    return [int.from_bytes(o[4 * i:4 * i + 4], 'little') for i in range(16)]


def unraw(buf, k):
    """the integer the fourteen limbs of element k stand for"""
    return sum(w << (28 * i) for i, w in enumerate(words(buf, k)[:14]))


# extremal field elements: the ends of the range, the middle, single high bits, alternating 28-bit limb patterns (the engine's limb size)
def extremes():
    lim = (1 << 28) - 1
    alt_a = sum((lim if i % 2 == 0 else 0) << (28 * i) for i in range(14)) % P
    alt_b = sum((lim if i % 2 == 1 else 0) << (28 * i) for i in range(14)) % P
    all_ones_limbs = sum(lim << (28 * i) for i in range(13))           # 13 saturated limbs, below p
    return [P - 1, 0, 1, (P - 1) // 2, (P + 1) // 2, (1 << 380) + 0x123456789abcdef, (1 << 380) - 1, P - 2, 2, alt_a, alt_b, all_ones_limbs,
            (1 << 379) + (1 << 28) - 1, P - (1 << 28), 3 * (P // 4)]


EXT = extremes()
LIMB_PATTERNS = EXT[9:12]      # alternating (either parity) and saturated limbs


@functools.lru_cache(maxsize=None)
def inverse_inputs():
    """the inversion routines' inputs: any representative below 2^392 -- random values below p and of random bit length, powers of two, all-ones, values next to p, tiny ones,
    unreduced ones and zero (3,171 values)"""
    rnd = random.Random(381)
    xs = [rnd.randrange(1, P) for _ in range(500)] + [rnd.randrange(1, 1 << rnd.randrange(1, 392)) for _ in range(1500)]
    xs += [1 << i for i in range(392)] + [(1 << i) - 1 for i in range(1, 392)] + [P - (1 << i) for i in range(380)]
    xs += [1, 2, P - 1, 0, 5 * P + 3, (1 << 391) + 12345, P + 1, 2 * P - 1]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def pow_inputs():
    """the Fp exponentiations' inputs, any representative below 16 p (the kernels' stated contract): the structured values first -- powers of two and all-ones up to 2^384, values
    next to p, every multiple of p below 16 p with 0, 1, 2, p - 1, p - 2 added, the alternating and saturated limb patterns --, then random values below 16 p, then the values
    the simulator test has always run (random values below p, (p + 1) / 2, 2^381 - 1 - p, 3 p + 5, 15 p + 7)"""
    xs = [1 << i for i in range(385)] + [(1 << i) - 1 for i in range(1, 385)] + [P - (1 << i) for i in range(380)]
    xs += [k * P + d for k in range(16) for d in (0, 1, 2, P - 1, P - 2)]
    xs += LIMB_PATTERNS
    rnd = random.Random(16381)
    xs += [rnd.randrange(0, 16 * P) for _ in range(200)]
    rnd = random.Random(5381)
    xs += [rnd.randrange(0, P) for _ in range(40)] + [0, 1, 2, P - 1, P - 2, (1 << 380), (1 << 381) - 1 - P, 3 * P + 5, 15 * P + 7, (P + 1) // 2]
    assert all(0 <= x < 16 * P for x in xs)
    return tuple(xs)


N_POW_STRUCTURED = 385 + 384 + 380 + 80 + 3      # the structured head of pow_inputs(): what the prefix and rotation tests run


@functools.lru_cache(maxsize=None)
def fp2_pow_inputs():
    """the Fp2 exponentiations' inputs (c0, c1), both components any representative below 16 p: all ordered pairs of a pool of fourteen structured values, random pairs below 16 p,
    then the pairs the simulator test has always run"""
    pool = [0, 1, 2, P - 2, P - 1, P, P + 1, (P + 1) // 2, 15 * P + 7, 16 * P - 1, (1 << 384) - 1, 1 << 384, LIMB_PATTERNS[0], LIMB_PATTERNS[2]]
    pairs = [(a, b) for a in pool for b in pool]
    rnd = random.Random(16382)
    pairs += [(rnd.randrange(0, 16 * P), rnd.randrange(0, 16 * P)) for _ in range(60)]
    rnd = random.Random(25381)
    pairs += [(rnd.randrange(0, P), rnd.randrange(0, P)) for _ in range(12)] + [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (5, 0), (0, 7), (15 * P + 3, 14 * P + 9), (P - 1, 1)]
    assert all(0 <= c < 16 * P for pr in pairs for c in pr)
    return tuple(pairs)


N_FP2_STRUCTURED = 14 * 14


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2pow(a, e):
    """square-and-multiply on Python integers"""
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2mul(r, r)
        if bit == '1':
            r = f2mul(r, a)
    return r


R_INV = pow(R, -1, P)


def inverse_expected(x):
    """what the inversion kernels' output is congruent to: x^-1 R^2 (the inverse of a Montgomery-form value in Montgomery form), 0 for x = 0 mod p"""
    return (pow(x % P, -1, P) * R * R) % P if x % P else 0


def pow_expected(x, which):
    """a^e R for the element a = x R^-1 a raw value x stands for"""
    return (pow((x * R_INV) % P, EXPONENTS[which], P) * R) % P


def fp2_pow_expected(pair, which):
    w = f2pow(((pair[0] * R_INV) % P, (pair[1] * R_INV) % P), EXPONENTS[which])
    return ((w[0] * R) % P, (w[1] * R) % P)


def tower_elements(ncoef, mixtures=40, seed=12):
    """elements of Fp^ncoef (coefficient lists) built from the extremes: every coefficient the same extreme, alternating p - 1 / 0 (either phase), p - 1 / 1, a cycle of
    six extremes, a single non-zero coefficient at either end, seeded random mixtures; the zero element last (callers that cannot take it drop it)"""
    if ncoef == 1:
        return [[v] for v in EXT if v] + [[0]]
    cases = [[v] * ncoef for v in EXT if v]
    cases.append([P - 1 if i % 2 == 0 else 0 for i in range(ncoef)])
    cases.append([0 if i % 2 == 0 else P - 1 for i in range(ncoef)])
    cases.append([P - 1 if i % 2 == 0 else 1 for i in range(ncoef)])
    cases.append([[(P - 1) // 2, P - 1, 1, 0, P - 2, 2][i % 6] for i in range(ncoef)])
    cases.append([0] * (ncoef - 1) + [P - 1])
    cases.append([P - 1] + [0] * (ncoef - 1))
    rnd = random.Random(seed)
    for _ in range(mixtures):
        cases.append([rnd.choice(EXT) for _ in range(ncoef)])
    return [c for c in cases if any(c)] + [[0] * ncoef]
