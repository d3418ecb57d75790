"""The doubling-and-add steps of the batched MSM (csrc/programs.h XP_DBLADD_G1 / _G2: acc <- 2 acc + T on raw projective points, in place) on the host simulator, without a GPU:
the static verifier, (acc, T) pairs against the oracle -- identity accumulator, identity slice, both, T = -2 acc (the identity comes out), T = 2 acc (the addition doubles),
T = acc, T = -acc --, and the translated form of the programs' ahead-of-time kernels.  The simulator's numbered entry points for programs outside the registry stop at the four
Horner steps of poly_eval; these two are reached by name."""
import ctypes as C
import random
import pytest
import vmsim_py
from vmsim_py import RAW, P_MOD, raw_elem, buf

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAMES = ['dbladd_g1', 'dbladd_g2']
# (a, t): acc = [a]G (0: the identity), slice T = [t]G (0: the identity); expected [(2 a + t) mod r]G
PAIRS = [(5, 7), (0, 7), (5, 0), (0, 0), (5, R - 10), (5, 10), (5, 5), (5, R - 5), (R - 1, 2), (R - 1, 1), ((R + 1) // 2, R - 1), (123456789, R - 2 * 123456789),
         (0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321)]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_extra_verify_named.argtypes = [C.c_char_p]
    lib.nbls_sim_extra_run_named.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
    return lib


def raw_point(oracle, k, g2, rnd):
    """[k]G as a raw projective point, multiplied through by a random z (any representative must do); k = 0 mod r: the identity (0 : y : 0) with a random y"""
    nf = 2 if g2 else 1
    rand = lambda: [rnd.randrange(1, P_MOD)] + [rnd.randrange(P_MOD) for _ in range(nf - 1)]
    if k % R == 0:
        return b''.join(raw_elem(v) for v in [0] * nf + rand() + [0] * nf)
    aff = (oracle.g2_mul(oracle.g2_generator(), k % R) if g2 else oracle.g1_mul(oracle.g1_generator(), k % R))[1]
    w = [int.from_bytes(aff[48 * i:48 * i + 48], 'big') for i in range(2 * nf)]
    z = rand()
    if g2:
        mul = lambda a, b: [(a[0] * b[0] - a[1] * b[1]) % P_MOD, (a[0] * b[1] + a[1] * b[0]) % P_MOD]
    else:
        mul = lambda a, b: [a[0] * b[0] % P_MOD]
    return b''.join(raw_elem(v) for v in mul(w[:nf], z) + mul(w[nf:], z) + z)


def steps(sim, oracle, name, pairs, aot=0):
    """one launch over the pairs -> (affine wire bytes per item, status per item: 1 = the zero point), through the simulator's norm / inversion / to-affine programs"""
    g2 = name.endswith('g2')
    p, sz, pre = (6 * RAW, 192, 'G2') if g2 else (3 * RAW, 96, 'G1')
    n = len(pairs)
    rnd = random.Random(len(name) * 100 + n + aot)
    acc = buf(b''.join(raw_point(oracle, a, g2, rnd) for a, _ in pairs))
    sl = buf(b''.join(raw_point(oracle, t, g2, rnd) for _, t in pairs))
    before = sl.raw
    ptrs, strides = (C.c_void_p * 8)(), (C.c_uint64 * 8)()
    for k, b in ((3, acc), (4, sl)):
        ptrs[k] = C.cast(b, C.c_void_p)
        strides[k] = p
    assert sim.nbls_sim_extra_run_named(name.encode(), aot, n, ptrs, strides) == 0
    assert sl.raw == before      # the slice is read only: the accumulator is the one buffer written
    N, NI, out, st = buf(RAW * n), buf(RAW * n), buf(sz * n), buf(n)
    vmsim_py.run(sim, pre + '_NORM', n, {3: (acc, p), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(n), N, NI)
    vmsim_py.run(sim, pre + '_TO_AFFINE', n, {3: (acc, p), 4: (NI, RAW), 2: (out, sz), 7: (st, 1)})
    return [out.raw[sz * i:sz * i + sz] for i in range(n)], list(st.raw[:n])


def expected(oracle, pairs, g2):
    want = []
    for a, t in pairs:
        s = (2 * a + t) % R
        want.append(None if s == 0 else (oracle.g2_mul(oracle.g2_generator(), s) if g2 else oracle.g1_mul(oracle.g1_generator(), s))[1])
    return want


def check(got, st, want):
    assert sum(w is None for w in want) >= 3 and any(w is not None for w in want)
    for i, w in enumerate(want):
        if w is None:
            assert st[i] == 1 and got[i] == bytes(len(got[i])), i
        else:
            assert st[i] == 0 and got[i] == w, i


@pytest.mark.parametrize('name', NAMES)
def test_the_programs_verify(sim, name):
    assert sim.nbls_sim_extra_verify_named(name.encode()) == 0
    assert sim.nbls_sim_extra_verify_named(b'dbladd_g3') == -1 and sim.nbls_sim_extra_verify_named(None) == -1
    ptrs, strides = (C.c_void_p * 8)(), (C.c_uint64 * 8)()
    assert sim.nbls_sim_extra_run_named(b'g1_add2', 0, 1, ptrs, strides) == -1      # a numbered program is not an extra one
    # the numbered entry points still end at the four Horner steps
    assert sim.nbls_sim_extra_count() == 4 and sim.nbls_sim_extra_verify(4) == -1


@pytest.mark.parametrize('name', NAMES)
def test_steps_against_the_oracle(sim, oracle, name):
    got, st = steps(sim, oracle, name, PAIRS)
    check(got, st, expected(oracle, PAIRS, name.endswith('g2')))


@pytest.mark.parametrize('name', NAMES)
def test_translated_form_gives_the_same_points(sim, oracle, name):
    """the step bodies of the program's ahead-of-time kernel (nbls_aot_dbladd_g1 / _g2) on the host; -2 would mean the program has no kernel in the simulator's table, -3 that
    its signatures are not in the table"""
    got, st = steps(sim, oracle, name, PAIRS, aot=1)
    check(got, st, expected(oracle, PAIRS, name.endswith('g2')))


def test_a_chain_is_a_scalar_multiplication(sim, oracle):
    """what the pipeline does with the step: acc <- 2 acc + T_j from the top bit down, T_j = P where bit j of k is set and the identity elsewhere, gives [k]P"""
    k = 0b1011001110001
    rnd = random.Random(7)
    p = 3 * RAW
    acc = buf(raw_point(oracle, 0, False, rnd))
    ptrs, strides = (C.c_void_p * 8)(), (C.c_uint64 * 8)()
    ptrs[3] = C.cast(acc, C.c_void_p)
    strides[3] = strides[4] = p
    for j in reversed(range(k.bit_length())):
        t = buf(raw_point(oracle, 9 if k >> j & 1 else 0, False, rnd))
        ptrs[4] = C.cast(t, C.c_void_p)
        assert sim.nbls_sim_extra_run_named(b'dbladd_g1', 0, 1, ptrs, strides) == 0
    N, NI, out, st = buf(RAW), buf(RAW), buf(96), buf(1)
    vmsim_py.run(sim, 'G1_NORM', 1, {3: (acc, p), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(1), N, NI)
    vmsim_py.run(sim, 'G1_TO_AFFINE', 1, {3: (acc, p), 4: (NI, RAW), 2: (out, 96), 7: (st, 1)})
    assert st.raw[0] == 0 and out.raw == oracle.g1_mul(oracle.g1_generator(), 9 * k)[1]
