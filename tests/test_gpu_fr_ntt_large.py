"""Transforms of more than 2^12 elements on the GPU (-m gpu): nbls_fr_ntt_large and nbls_fr_ntt_dev against the one-workgroup transform under forced splits, against Python
integers (fr_ntt_large_cases.py) at 2^13 .. 2^15, against the composition of two nbls_fr_ntt calls at 2^18 and against the closed form of a sparse polynomial at 2^22.
Outputs are pre-filled with 0x7f: a byte the call does not write shows."""
import ctypes as C
import hashlib
import importlib
import random
import numpy as np
import pytest
from kzg_cases import R, M256
from kzg_cells_cases import coset_shift, rows
from fr_ntt_large_cases import compose_to_evals, compose_to_coeffs, block_shift, sparse_eval

pytestmark = pytest.mark.gpu
EINVAL, NON_CANONICAL, ZERO_SHIFT = -1, 21, 5


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    e = pkg.Engine(0)
    yield e
    e.set_ntt_plan(0, 0)


def large(eng, log2_n, to_evals, raw, shifts=None, want_rc=0):
    """nbls_fr_ntt_large on pre-filled buffers -> (bytes, status list)"""
    n = len(raw) // (32 << log2_n)
    out, st = C.create_string_buffer(b'\x7f' * max(len(raw), 1), max(len(raw), 1)), C.create_string_buffer(b'\x7f' * max(n, 1), max(n, 1))
    assert eng.lib.nbls_fr_ntt_large(eng.h, log2_n, 1 if to_evals else 0, n, raw, shifts, out, st) == want_rc
    return out.raw[:len(raw)], list(st.raw[:n])


def small(eng, log2_n, to_evals, raw, shifts=None):
    """Engine.fr_ntt -> (bytes, status list)"""
    n = len(raw) // (32 << log2_n)
    got, st = eng.fr_ntt(log2_n, raw, to_evals, None if shifts is None else [shifts[32 * i:32 * i + 32] for i in range(n)])
    return b''.join(b''.join(r) for r in got), st


def random_rows(log2_n, n, seed):
    """n polynomials of random canonical elements: the top byte masked to 0x3f keeps every element below r"""
    a = np.random.default_rng(seed).integers(0, 256, size=(n << log2_n, 32), dtype=np.uint8)
    a[:, 0] &= 0x3f
    return a.tobytes()


# ---- 1. forced splits against the one-workgroup transform
@pytest.mark.parametrize('log2_n', [2, 5, 9, 12])
def test_forced_splits_equal_the_one_workgroup_transform(eng, log2_n):
    n, row = 5, 32 << log2_n
    data = bytearray(random_rows(log2_n, n, 100 + log2_n))
    data[row + 32 * ((1 << log2_n) - 1):2 * row] = R.to_bytes(32, 'big')          # row 1: its last element is r
    shifts = rows([7, 11, coset_shift(log2_n), 0, R - 1])                           # row 3: a zero shift
    data = bytes(data)
    want = {d: small(eng, log2_n, d, data, shifts) for d in (True, False)}
    assert want[True][1] == [0, NON_CANONICAL, 0, ZERO_SHIFT, 0] and want[True][0][row:2 * row] == bytes(row)
    try:
        for t in (1, 3, 6):
            for p in (1, 2, 0):
                eng.set_ntt_plan(t, p)
                for d in (True, False):
                    assert large(eng, log2_n, d, data, shifts) == want[d], (t, p, d)
    finally:
        eng.set_ntt_plan(0, 0)


# ---- 2. the default plan (and three global launches) against Python integers
@pytest.mark.parametrize('log2_n,n,pass_bits', [(13, 2, 0), (14, 1, 0), (15, 1, 1)])
def test_default_plan_against_python(eng, log2_n, n, pass_bits):
    rnd = random.Random(200 + log2_n)
    polys = [[rnd.randrange(R) for _ in range(1 << log2_n)] for _ in range(n)]
    polys[0][0], polys[0][-1] = 0, R - 1
    s = [rnd.randrange(1, R), 1][:n]
    data, sh = b''.join(rows(p) for p in polys), rows(s)
    try:
        eng.set_ntt_plan(0, pass_bits)
        for d, ref in ((True, compose_to_evals), (False, compose_to_coeffs)):
            got, st = large(eng, log2_n, d, data, sh)
            assert st == [0] * n
            assert got == b''.join(rows(ref(p, log2_n, 12, x)) for p, x in zip(polys, s)), d
    finally:
        eng.set_ntt_plan(0, 0)
    # the binding, both argument forms
    got_b, st_b = eng.fr_ntt_large(log2_n, data, True, sh)
    got_l, st_l = eng.fr_ntt_large(log2_n, polys, True, s)
    assert st_b == st_l == [0] * n and got_b == b''.join(b''.join(r) for r in got_l) == large(eng, log2_n, True, data, sh)[0]


# ---- 3. dense at 2^18 against the composition of two nbls_fr_ntt calls (fact 2 and fact 3 with the calls that were there before)
def compose_on_device(eng, log2_n, t, to_evals, raw):
    k = log2_n - t
    sb = [block_shift(log2_n, t, b) for b in range(1 << k)]

    def columns(a):          # (2^k rows, 2^t columns) -> every column through the transform of size 2^k
        cols = np.ascontiguousarray(a.reshape(1 << k, 1 << t, 32).transpose(1, 0, 2)).tobytes()
        got, st = small(eng, k, to_evals, cols)
        assert not any(st)
        return np.ascontiguousarray(np.frombuffer(got, dtype=np.uint8).reshape(1 << t, 1 << k, 32).transpose(1, 0, 2))

    def tails(a):
        got, st = small(eng, t, to_evals, a.tobytes(), rows(sb))
        assert not any(st)
        return np.frombuffer(got, dtype=np.uint8)

    a = np.frombuffer(raw, dtype=np.uint8)
    return (tails(columns(a)) if to_evals else columns(tails(a))).tobytes()


def test_dense_2_to_18_equals_the_composition(eng):
    log2_n = 18
    data = random_rows(log2_n, 1, 300)
    for d in (True, False):
        got, st = large(eng, log2_n, d, data)
        assert st == [0]
        assert got == compose_on_device(eng, log2_n, 12, d, data), d


# ---- 4. sparse at 2^22 against the closed form
def test_sparse_2_to_22_against_the_closed_form(eng):
    log2_n, shift = 22, 7
    n = 1 << log2_n
    terms = [(0, 5), (4095 * (1 << 10) + 1, R - 3), (1 << 21, 0x1234567890abcdef), (n - 1, R - 1)]
    coef = bytearray(32 * n)
    for e, c in terms:
        coef[32 * e:32 * e + 32] = c.to_bytes(32, 'big')
    coef, sh = bytes(coef), rows([shift])
    rnd = random.Random(400)
    # every power of two and its predecessor: the borders of the tails and of every tile any plan has
    at = {0, n - 1, 4095, 4096} | {(1 << b) - 1 for b in range(1, 23)} | {1 << b for b in range(22)} | {4095 << 10, (4095 << 10) + 1}
    while len(at) < 256:
        at.add(rnd.randrange(n))
    want = {j: sparse_eval(terms, log2_n, j, shift).to_bytes(32, 'big') for j in at}
    try:
        for pass_bits in (0, 5):
            eng.set_ntt_plan(0, pass_bits)
            vals, st = large(eng, log2_n, True, coef, sh)
            assert st == [0]
            for j in sorted(at):
                assert vals[32 * j:32 * j + 32] == want[j], (pass_bits, j)
            back, st = large(eng, log2_n, False, vals, sh)
            assert st == [0] and hashlib.sha256(back).digest() == hashlib.sha256(coef).digest(), pass_bits
    finally:
        eng.set_ntt_plan(0, 0)


# ---- 5. the device-resident call on torch buffers
@pytest.mark.parametrize('log2_n,tail', [(13, 0), (9, 4)])
def test_device_resident_call(eng, log2_n, tail):
    import torch
    n, row = 3, 32 << log2_n
    data, sh = random_rows(log2_n, n, 500 + log2_n), rows([3, 1, coset_shift(log2_n)])
    other = random_rows(log2_n, 1, 600 + log2_n)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    side = torch.cuda.Stream()
    try:
        eng.set_ntt_plan(tail, 0)
        for d in (True, False):
            want, want_st = large(eng, log2_n, d, data, sh)
            want_other = large(eng, log2_n, d, other)
            assert want_st == [0] * n
            d_in, d_sh = dev(data), dev(sh)
            for stream in (None, side):
                handle = None if stream is None else stream.cuda_stream
                # out of place, the status on the device
                d_out, d_st = torch.full((n * row,), 0x7f, dtype=torch.uint8, device='cuda'), torch.full((n,), 0x7f, dtype=torch.uint8, device='cuda')
                torch.cuda.synchronize()
                eng.fr_ntt_dev(log2_n, n, d_in.data_ptr(), d, d_out.data_ptr(), d_sh.data_ptr(), d_st.data_ptr(), stream=handle)
                # a host-buffer call behind it on the same context: it uses the same scratch, and waits for the stream
                assert large(eng, log2_n, d, other) == want_other
                torch.cuda.synchronize()
                assert d_out.cpu().numpy().tobytes() == want and d_st.cpu().tolist() == [0] * n and d_in.cpu().numpy().tobytes() == data
                # in place, no status
                d_io = dev(data)
                torch.cuda.synchronize()
                eng.fr_ntt_dev(log2_n, n, d_io.data_ptr(), d, d_io.data_ptr(), d_sh.data_ptr(), None, stream=handle)
                torch.cuda.synchronize()
                assert d_io.cpu().numpy().tobytes() == want
            # partial overlap
            big = torch.zeros((2 * n * row,), dtype=torch.uint8, device='cuda')
            for off in (32, row, n * row - 32):
                assert eng.lib.nbls_fr_ntt_dev(eng.h, log2_n, int(d), n, big.data_ptr(), None, big.data_ptr() + off, None, None) == EINVAL
                assert eng.lib.nbls_fr_ntt_dev(eng.h, log2_n, int(d), n, big.data_ptr() + off, None, big.data_ptr(), None, None) == EINVAL
            assert eng.lib.nbls_fr_ntt_dev(eng.h, log2_n, int(d), n, big.data_ptr() + 8, None, big.data_ptr() + n * row, None, None) == EINVAL          # alignment
            torch.cuda.synchronize()
            assert not big.any().item()
    finally:
        eng.set_ntt_plan(0, 0)


# ---- 6. refusals, the argument rules, a context whose first call is the large one
@pytest.mark.parametrize('to_evals', [True, False])
def test_refusals_at_2_to_13(eng, to_evals):
    log2_n, n = 13, 3
    N, row = 1 << log2_n, 32 << log2_n
    good, shifts = random_rows(log2_n, n, 700), [3, 11, coset_shift(log2_n)]
    clean, st = large(eng, log2_n, to_evals, good, rows(shifts))
    assert st == [0, 0, 0]
    zero = bytes(row)

    def check(data, sh, code):
        got, st = large(eng, log2_n, to_evals, data, sh)
        assert st == [0, code, 0]
        assert got[:row] == clean[:row] and got[row:2 * row] == zero and got[2 * row:] == clean[2 * row:]
    # an element >= r in the LAST block of the middle polynomial
    at = row + 32 * (N - 2)
    for bad in (R, M256):
        check(good[:at] + bad.to_bytes(32, 'big') + good[at + 32:], rows(shifts), NON_CANONICAL)
    for bad, code in ((R, NON_CANONICAL), (M256, NON_CANONICAL), (0, ZERO_SHIFT)):
        check(good, rows(shifts[:1]) + bad.to_bytes(32, 'big') + rows(shifts[2:]), code)
    # non-canonical before zero
    check(good[:row] + R.to_bytes(32, 'big') + good[row + 32:], rows([shifts[0], 0, shifts[2]]), NON_CANONICAL)


def test_argument_rules_and_a_fresh_context(pkg, eng):
    log2_n = 13
    data = random_rows(log2_n, 1, 800)
    x = bytes(64)
    for k in (0, 25):
        out = C.create_string_buffer(64)
        assert eng.lib.nbls_fr_ntt_large(eng.h, k, 1, 1, x, None, out, None) == EINVAL and out.raw == bytes(64)
    out = C.create_string_buffer(64)
    assert eng.lib.nbls_fr_ntt_large(eng.h, log2_n, 1, (1 << 11) + 1, x, None, out, None) == EINVAL          # (n << log2_n) = 2^24 + 2^log2_n
    assert eng.lib.nbls_fr_ntt_large(eng.h, log2_n, 2, 1, x, None, out, None) == EINVAL
    assert eng.lib.nbls_fr_ntt_large(eng.h, log2_n, 1, 1, None, None, out, None) == EINVAL
    assert eng.lib.nbls_fr_ntt_large(eng.h, log2_n, 1, 0, None, None, None, None) == 0 and out.raw == bytes(64)          # n = 0
    assert eng.lib.nbls_fr_ntt_dev(eng.h, log2_n, 1, 0, None, None, None, None, None) == 0
    want = {d: large(eng, log2_n, d, data) for d in (True, False)}
    other = pkg.Engine(0)          # its tables are built by the call below
    assert large(other, log2_n, False, data) == want[False]
    assert large(other, log2_n, True, data) == want[True]
