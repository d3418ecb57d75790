"""nbls_verify_multiple without a GPU: the 64-bit G1 ladder P_G1_MUL64 and the weight derivation (rlc_weights.h) on the simulator against the oracle and hashlib, and the
entry point exported by libnbls.so and declared by the binding."""
import ctypes as C
import hashlib
import importlib
import os
import random
import subprocess
import vmsim_py
from goldenio import hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
RAW = vmsim_py.RAW
G1_MUL64 = len(vmsim_py.PROGS)        # appended after the last program vmsim_py names (programs.h: just before P_COUNT)


def _run(sim, prog, n, bufs):
    ptrs = (C.c_void_p * 8)()
    strides = (C.c_uint64 * 8)()
    for k, (b, s) in bufs.items():
        ptrs[k] = C.cast(b, C.c_void_p)
        strides[k] = s
    assert sim.nbls_sim_run(prog, C.c_uint(n), ptrs, strides) == 0


def _mul64(sim, pts96, scalars32):
    """the key chain of pipelines_multi_verify.cpp on the simulator: P_G1_MUL64 -> inversion -> P_G1_TO_AFFINE (as vmsim_py.point_mul)"""
    n = len(scalars32) // 32
    buf = vmsim_py.buf
    Pj, N, NI, out, st = buf(3 * RAW * n), buf(RAW * n), buf(RAW * n), buf(96 * n), buf(n)
    _run(sim, G1_MUL64, n, {0: (buf(pts96), 96), 2: (buf(scalars32), 32), 3: (Pj, 3 * RAW), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(n), N, NI)
    vmsim_py.run(sim, 'G1_TO_AFFINE', n, {3: (Pj, 3 * RAW), 4: (NI, RAW), 2: (out, 96), 7: (st, 1)})
    return out.raw, st.raw


def test_program_registered_and_verified():
    sim = vmsim_py.load()
    assert sim.nbls_sim_program_count() == len(vmsim_py.PROGS) + 1
    msg = C.create_string_buffer(256)
    assert sim.nbls_sim_verify(G1_MUL64, msg, 256) == 0, msg.value.decode()


def test_g1_mul64_against_oracle(oracle, golden):
    sim = vmsim_py.load()
    rnd = random.Random(64)
    ks = [1 << 63, (1 << 63) + 1, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA] + [rnd.getrandbits(64) | (1 << 63) for _ in range(4)]
    g1 = oracle.g1_generator()
    others = [hx(p['aff']) for p in golden['g1pts'][:3]]
    pts = [g1] + others
    cases = [(pts[i % len(pts)], k) for i, k in enumerate(ks)] + [(p, ks[2]) for p in pts] + [(p, ks[3]) for p in others]
    # the weights as the pipeline stores them: 24 zero bytes, then the 64-bit value
    out, st = _mul64(sim, b''.join(p for p, _ in cases), b''.join(k.to_bytes(32, 'big') for _, k in cases))
    for i, (p, k) in enumerate(cases):
        assert st[i] == 0
        assert out[96 * i:96 * i + 96] == oracle.g1_mul(p, k)[1], (i, hex(k))


def test_g1_mul64_reads_only_the_low_eight_bytes(oracle):
    """bytes 0..23 of the scalar are not part of the 64-bit ladder's input"""
    sim = vmsim_py.load()
    g1 = oracle.g1_generator()
    k = 0xC0FFEE0123456789
    out, st = _mul64(sim, g1, (0xFF << 200 | k).to_bytes(32, 'big'))
    assert st[0] == 0 and out == oracle.g1_mul(g1, k)[1]


def test_weights_against_hashlib():
    sim = vmsim_py.load()
    sim.nbls_sim_rlc_weight.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    for seed in (bytes(range(32)), hashlib.sha256(b'another seed').digest()):
        for i in (0, 1, 255, 256, 65535, 65536, (1 << 32) + 1):
            out = C.create_string_buffer(32)
            sim.nbls_sim_rlc_weight(seed, i, out)
            h = hashlib.sha256(seed + i.to_bytes(8, 'big')).digest()
            r = int.from_bytes(h[:8], 'big') | (1 << 63)
            assert out.raw == r.to_bytes(32, 'big'), (seed.hex(), i)
            assert out.raw[:24] == bytes(24) and out.raw[24] & 0x80


def test_entry_point_exported_and_bound():
    subprocess.check_call(['make', '-s', '-C', os.path.join(PKG, 'csrc'), '../libnbls.so'])
    lib = C.CDLL(os.path.join(PKG, 'libnbls.so'))
    assert hasattr(lib, 'nbls_verify_multiple')
    assert lib.nbls_abi_version() == 5
    pkg = importlib.import_module('noble-bls12-381_amd')
    bound = pkg.load_library()
    assert bound.nbls_verify_multiple.argtypes is not None and len(bound.nbls_verify_multiple.argtypes) == 11
    assert hasattr(pkg.Engine, 'verify_multiple')
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ST_NOT_VERIFIED 9' in src and '#define NBLS_ABI_VERSION 5' in src
