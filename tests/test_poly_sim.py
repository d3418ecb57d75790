"""The Horner-step programs of nbls_g*_poly_eval (csrc/programs.h ExtraProg: acc <- [x]acc + A on raw projective points, a 16-bit and a 256-bit form per group) on the host
simulator, without a GPU: the static verifier, (acc, x, A) triples against the oracle -- identity accumulator, identity coefficient, x = 0, [x]acc = -A, [x]acc = A, the edges of
both widths --, the short form's reading of the low two bytes only, and the translated form of the programs' ahead-of-time kernels.  The programs live outside the numbered
registry, so the simulator's entry points for them are bound here."""
import ctypes as C
import random
import pytest
import vmsim_py
from vmsim_py import RAW, P_MOD, raw_elem, buf

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NAMES = ['poly_g1_16', 'poly_g1_256', 'poly_g2_16', 'poly_g2_256']
# (a, x, b): acc = [a]G (0: the identity), identifier x, coefficient [b]G (0: the identity); expected [(x a + b) mod r]G
COMMON = [(5, 3, 7), (0, 9, 7), (5, 3, 0), (5, 0, 7), (0, 0, 0), (5, 3, R - 15), (5, 3, 15), (R - 1, 2, 2), (123456789, 1, R - 123456789)]
SHORT = COMMON + [(11, (1 << 16) - 1, 13), (R - 2, (1 << 16) - 1, 1), (7, 1 << 15, 0)]
FULL = COMMON + [(11, 1 << 16, 13), (11, R - 1, 13), (11, R - 1, 11), (11, R, 13), (11, R + 1, 13), (11, (1 << 256) - 1, 13), (3, 1 << 64, 5), (9, (1 << 255) + 12345, R - 1)]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_extra_name.restype = C.c_char_p
    lib.nbls_sim_extra_name.argtypes = [C.c_int]
    lib.nbls_sim_extra_verify.argtypes = [C.c_int]
    lib.nbls_sim_extra_run.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
    return lib


def xp(sim, name):
    names = [sim.nbls_sim_extra_name(i).decode() for i in range(sim.nbls_sim_extra_count())]
    return names.index(name)


def run_extra(sim, name, n, bufs, aot=0):
    ptrs = (C.c_void_p * 8)()
    strides = (C.c_uint64 * 8)()
    for k, (b, s) in bufs.items():
        ptrs[k] = C.cast(b, C.c_void_p)
        strides[k] = s
    return sim.nbls_sim_extra_run(xp(sim, name), aot, n, ptrs, strides)


def raw_point(oracle, k, g2, rnd):
    """[k]G as a raw projective point, multiplied through by a random z (any representative must do); k = 0: the identity (0 : z : 0)"""
    nf = 2 if g2 else 1
    if k % R == 0:
        x, y, z = [0] * nf, [rnd.randrange(1, P_MOD)] + [rnd.randrange(P_MOD)] * (nf - 1), [0] * nf
    else:
        aff = (oracle.g2_mul(oracle.g2_generator(), k % R) if g2 else oracle.g1_mul(oracle.g1_generator(), k % R))[1]
        w = [int.from_bytes(aff[48 * i:48 * i + 48], 'big') for i in range(2 * nf)]
        x, y, z = w[:nf], w[nf:], [1] + [0] * (nf - 1)
        zz = [rnd.randrange(1, P_MOD)] + [rnd.randrange(P_MOD)] * (nf - 1)
        if g2:
            mul2 = lambda a, b: [(a[0] * b[0] - a[1] * b[1]) % P_MOD, (a[0] * b[1] + a[1] * b[0]) % P_MOD]
            x, y, z = mul2(x, zz), mul2(y, zz), zz
        else:
            x, y, z = [x[0] * zz[0] % P_MOD], [y[0] * zz[0] % P_MOD], zz
    return b''.join(raw_elem(v) for v in x + y + z)


def horner_steps(sim, oracle, name, triples, ids=None, aot=0):
    """one launch over the triples -> (affine wire bytes per item, status per item: 1 = the zero point), through the simulator's norm / inversion / to-affine programs"""
    g2 = 'g2' in name
    p, sz, pre = ((6 * RAW, 192, 'G2') if g2 else (3 * RAW, 96, 'G1'))
    n = len(triples)
    rnd = random.Random(len(name) * 1000 + n)
    acc = buf(b''.join(raw_point(oracle, a, g2, rnd) for a, _, _ in triples))
    co = buf(b''.join(raw_point(oracle, b, g2, rnd) for _, _, b in triples))
    xs = buf(b''.join((x.to_bytes(32, 'big') for _, x, _ in triples) if ids is None else ids))
    assert run_extra(sim, name, n, {2: (xs, 32), 3: (acc, p), 4: (co, p)}, aot) == 0
    N, NI, out, st = buf(RAW * n), buf(RAW * n), buf(sz * n), buf(n)
    vmsim_py.run(sim, pre + '_NORM', n, {3: (acc, p), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(n), N, NI)
    vmsim_py.run(sim, pre + '_TO_AFFINE', n, {3: (acc, p), 4: (NI, RAW), 2: (out, sz), 7: (st, 1)})
    return [out.raw[sz * i:sz * i + sz] for i in range(n)], list(st.raw[:n])


def expected(oracle, triples, g2):
    want = []
    for a, x, b in triples:
        s = ((x % R) * a + b) % R
        want.append(None if s == 0 else (oracle.g2_mul(oracle.g2_generator(), s) if g2 else oracle.g1_mul(oracle.g1_generator(), s))[1])
    return want


def check(got, st, want):
    assert any(w is None for w in want) and any(w is not None for w in want)
    for i, w in enumerate(want):
        if w is None:
            assert st[i] == 1, i
        else:
            assert st[i] == 0 and got[i] == w, i


def test_the_four_programs_exist_and_verify(sim):
    assert [sim.nbls_sim_extra_name(i).decode() for i in range(sim.nbls_sim_extra_count())] == NAMES
    for i in range(len(NAMES)):
        assert sim.nbls_sim_extra_verify(i) == 0, NAMES[i]
    assert sim.nbls_sim_extra_verify(len(NAMES)) == -1 and sim.nbls_sim_extra_name(len(NAMES)) is None
    ptrs, strides = (C.c_void_p * 8)(), (C.c_uint64 * 8)()
    assert sim.nbls_sim_extra_run(len(NAMES), 0, 1, ptrs, strides) == -1
    # the numbered registry did not grow: the simulator's own entry still refuses everything from its count on
    assert sim.nbls_sim_run(sim.nbls_sim_program_count(), C.c_uint(1), ptrs, strides) == -1


@pytest.mark.parametrize('name', NAMES)
def test_steps_against_the_oracle(sim, oracle, name):
    triples = SHORT if name.endswith('_16') else FULL
    got, st = horner_steps(sim, oracle, name, triples)
    check(got, st, expected(oracle, triples, 'g2' in name))


@pytest.mark.parametrize('name', ['poly_g1_16', 'poly_g2_16'])
def test_the_short_form_reads_the_low_two_bytes(sim, oracle, name):
    triples = [(5, 3, 7), (11, (1 << 16) - 1, 13), (5, 0, 7), (9, 258, R - 1)]
    rnd = random.Random(16)
    noisy = [(rnd.getrandbits(240) << 16 | x).to_bytes(32, 'big') for _, x, _ in triples]
    assert all(n[:30] != bytes(30) for n in noisy)
    got, st = horner_steps(sim, oracle, name, triples, ids=noisy)
    want = expected(oracle, triples, 'g2' in name)
    assert st == [0] * len(triples) and got == want


@pytest.mark.parametrize('name', NAMES)
def test_translated_form_gives_the_same_bytes(sim, oracle, name):
    """the step bodies of the program's ahead-of-time kernel (nbls_aot_poly_g1 / _g2) on the host; -2 would mean the program has no kernel in the simulator's table, -3 that its
    signatures are not in the table"""
    triples = (SHORT if name.endswith('_16') else FULL)[:8] + [(11, (1 << 16) - 1, 13)]
    got, st = horner_steps(sim, oracle, name, triples, aot=1)
    assert (got, st) == horner_steps(sim, oracle, name, triples)
    check(got, st, expected(oracle, triples, 'g2' in name))
