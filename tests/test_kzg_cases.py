"""The helpers that test_gpu_kzg_adversarial.py builds its inputs from (kzg_cases.py), checked without a GPU: weight against the simulator's rlc_weight -- the code the
device compiles (rlc_weights.h) -- and Setup.tuple_for against Setup.commit / Setup.proof on polynomials."""
import ctypes as C
import hashlib
import random
import vmsim_py
from kzg_cases import R, TAU, ZERO48, Setup, b32, eval_roots, weight


def test_weight_is_the_simulators():
    sim = vmsim_py.load()
    sim.nbls_sim_rlc_weight.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    for seed in (bytes(range(32)), bytes(32), hashlib.sha256(b'kzg cases').digest()):
        for i in (0, 1, 255, 256, 599, 1 << 32, (1 << 64) - 1):
            out = C.create_string_buffer(32)
            sim.nbls_sim_rlc_weight(seed, i, out)
            assert out.raw == b32(weight(seed, i)), (seed.hex(), i)
            assert 1 << 63 <= weight(seed, i) < 1 << 64


def test_tuple_for_agrees_with_commit_and_proof(oracle):
    rnd = random.Random(700)
    setup = Setup(oracle)
    for _ in range(3):
        f = [rnd.randrange(R) for _ in range(4)]
        z = rnd.randrange(R)
        y, p = setup.proof(f, z, 2)
        s = (eval_roots(f, TAU, 2) - y) * pow(TAU - z, -1, R) % R          # the quotient at tau: the (s, z, y) of this opening
        assert y == eval_roots(f, z, 2) and s != 0
        assert setup.tuple_for(s, z, y) == (setup.commit(f, 2), z, y, p)
        assert setup.tuple_for(s + 1, z, y)[0] != setup.commit(f, 2)


def test_tuple_for_zero_points_and_pool(oracle):
    rnd = random.Random(701)
    setup = Setup(oracle)
    z, y = rnd.randrange(1, R), rnd.randrange(1, R)
    assert setup.tuple_for(0, z, y) == (setup.g1(y), z, y, ZERO48)          # a constant polynomial
    assert setup.tuple_for(0, z, 0) == (ZERO48, z, 0, ZERO48)
    s = rnd.randrange(1, R)
    assert setup.tuple_for(s, z, s * (z - TAU) % R)[0] == ZERO48            # c = 0 with a non-zero proof
    ts = setup.tuples_pooled(40, rnd, pool=4)
    assert len(ts) == 40 and len({t[3] for t in ts}) <= 4 and len({t[1] for t in ts}) == 40 and len({t[0] for t in ts}) == 40
    assert all(len(t[0]) == 48 and len(t[3]) == 48 and ZERO48 not in (t[0], t[3]) for t in ts)
