"""The Fr side of the FK20 cell proofs without a GPU: fr_fk_* of fr_exec.h -- the code kzg_fk20_scalars_kernel and kzg_fk20_matrix_kernel compile for the device -- on the
simulator (nbls_sim_kzg_fk20_scalars: workgroups of 256 lanes, the same stripes, elements and butterflies per lane, phase after phase; nbls_sim_kzg_fk20_matrix) against Python
integers (kzg_fk20_cases.py).  Bit-exact.

The sizes: M = 2, 4, 16, 64, 128, and every M at which the ownership of the scalars kernel changes.  Up to M = 256 a lane owns ONE butterfly of a stage and a workgroup
holds 512 / M stripes side by side (M = 2: one lane per stripe, 256 stripes); at M = 512 a workgroup holds exactly one stripe, still one butterfly per lane; from M = 1024 on
a lane owns M / 512 butterflies of its one stripe.  So 256, 512 and 1024 are run as well, and with c = 1, 2, 4, 8 and three blobs the stripes also end in the middle of a
workgroup (a workgroup's last stripes are then idle lanes that store nothing) and cross from one blob into the next inside one."""
import ctypes as C
import random
import pytest
import vmsim_py
from kzg_cases import R
from kzg_cells_cases import structured, rows
import kzg_fk20_cases as fk

# (log2_n, log2_cell): M = 2^(log2_n + 1 - log2_cell)
SHAPES = [(3, 3), (2, 1), (3, 0), (5, 2), (5, 0), (8, 3), (6, 0), (8, 1), (8, 0), (9, 0)]


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.nbls_sim_kzg_fk20_scalars.argtypes = [u, u, sz, vp, vp]
    lib.nbls_sim_kzg_fk20_matrix.argtypes = [u, vp]
    return lib


def ints(raw, k):
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'big') for i in range(k)]


def run_scalars(sim, log2_n, log2_cell, polys):
    n, per = len(polys), 2 << log2_n
    out = C.create_string_buffer(32 * n * per)
    assert sim.nbls_sim_kzg_fk20_scalars(log2_n, log2_cell, n, b''.join(rows(f) for f in polys), out) == 0
    v = ints(out.raw, n * per)
    return [v[i * per:(i + 1) * per] for i in range(n)]


def test_shapes_cover_the_sizes():
    assert sorted({1 << (a + 1 - b) for a, b in SHAPES}) == [2, 4, 16, 64, 128, 256, 512, 1024]


@pytest.mark.parametrize('log2_n,log2_cell', [s for s in SHAPES if s[0] <= 6])
def test_scalars_of_structured_polynomials(sim, log2_n, log2_cell):
    """every structured polynomial of the transform's tests, and a refused blob (its coefficients are all-zero, as the front ends leave them) between two of them"""
    rnd = random.Random(2000 + 16 * log2_n + log2_cell)
    cases = structured(log2_n, rnd)
    polys = [f for _, f in cases]
    polys.insert(2, [0] * (1 << log2_n))
    got = run_scalars(sim, log2_n, log2_cell, polys)
    for f, g in zip(polys, got):
        assert g == fk.scalars_flat(f, log2_n, log2_cell)
    assert not any(got[2])


@pytest.mark.parametrize('log2_n,log2_cell', [s for s in SHAPES if s[0] > 6])
def test_scalars_at_the_larger_sizes(sim, log2_n, log2_cell):
    """three blobs -- a random one, a refused one, X^(N-1) -- where the integer reference is costly: every entry of the first, a sample of the others"""
    rnd = random.Random(2100 + 16 * log2_n + log2_cell)
    N, c, np_, M, lm = fk.dims(log2_n, log2_cell)
    polys = [[rnd.randrange(R) for _ in range(N)], [0] * N, [0] * (N - 1) + [1]]
    got = run_scalars(sim, log2_n, log2_cell, polys)
    assert not any(got[1])
    w = [fk.pos_root(i, lm) for i in range(M)]

    def entry(f, i, j):
        return sum(f[j + c * t] * pow(w[i], t, R) for t in range(np_)) % R

    picks = [(i, j) for i in sorted({0, 1, M // 2 - 1, M // 2, M - 1, rnd.randrange(M)}) for j in sorted({0, c - 1, rnd.randrange(c)})]
    for b in (0, 2):
        for i, j in picks:
            assert got[b][i * c + j] == entry(polys[b], i, j), (b, i, j)
    # the whole of the random blob through the transform's own integer reference: stripe j, zero-padded, to values in bit-reversed order
    from kzg_cells_cases import to_evals
    for j in range(c):
        want = to_evals([polys[0][j + c * t] for t in range(np_)] + [0] * np_, lm)
        assert [got[0][i * c + j] for i in range(M)] == want, j


@pytest.mark.parametrize('log2_n,log2_cell', [(3, 3), (2, 1), (3, 0), (5, 2), (6, 3), (5, 0), (6, 0)])
def test_matrix(sim, log2_n, log2_cell):
    _, _, _, M, lm = fk.dims(log2_n, log2_cell)
    out = C.create_string_buffer(32 * M * M)
    assert sim.nbls_sim_kzg_fk20_matrix(lm, out) == 0
    v = ints(out.raw, M * M)
    assert [v[k * M:(k + 1) * M] for k in range(M)] == fk.matrix(log2_n, log2_cell)


def test_refused_sizes(sim):
    out = C.create_string_buffer(64)
    assert sim.nbls_sim_kzg_fk20_scalars(0, 0, 1, bytes(32), out) == -1 and sim.nbls_sim_kzg_fk20_scalars(2, 3, 1, bytes(128), out) == -1
    assert sim.nbls_sim_kzg_fk20_scalars(12, 0, 1, None, None) == -1          # M = 2^13
    assert sim.nbls_sim_kzg_fk20_matrix(0, out) == -1 and sim.nbls_sim_kzg_fk20_matrix(12, out) == -1
    assert out.raw == bytes(64)


Z2 = 0xd201000000010000 ** 2 % R


def test_the_conversion_between_the_passes(sim, oracle):
    """endo_g1 (programs.h XP_ENDO_G1): a raw projective point -> the point and [z^2]P = (beta X, -Y, Z), the pair P_G1_MSM_PREP makes from affine bytes, for any
    representative; the identity (0 : y : 0) stays the identity in both halves"""
    from vmsim_py import RAW, buf
    from test_msm_batch_sim import raw_point
    sim.nbls_sim_extra_verify_named.argtypes = [C.c_char_p]
    sim.nbls_sim_extra_run_named.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
    assert sim.nbls_sim_extra_verify_named(b'endo_g1') == 0
    ks = [1, 5, 0, R - 1, 0x1234567890abcdef1234567890abcdef, 0]
    rnd, p, n = random.Random(20), 3 * RAW, 6
    src = buf(b''.join(raw_point(oracle, k, False, rnd) for k in ks))
    dst = buf(2 * p * n)
    before = src.raw
    ptrs, strides = (C.c_void_p * 8)(), (C.c_uint64 * 8)()
    ptrs[3], strides[3], ptrs[5], strides[5] = C.cast(src, C.c_void_p), p, C.cast(dst, C.c_void_p), 2 * p
    assert sim.nbls_sim_extra_run_named(b'endo_g1', 0, n, ptrs, strides) == 0 and src.raw == before
    N, NI, out, st = buf(RAW * 2 * n), buf(RAW * 2 * n), buf(96 * 2 * n), buf(2 * n)
    vmsim_py.run(sim, 'G1_NORM', 2 * n, {3: (dst, p), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(2 * n), N, NI)
    vmsim_py.run(sim, 'G1_TO_AFFINE', 2 * n, {3: (dst, p), 4: (NI, RAW), 2: (out, 96), 7: (st, 1)})
    for i, k in enumerate(ks):
        for half, s in enumerate((k, k * Z2 % R)):
            at = 2 * i + half
            if k == 0:
                assert st.raw[at] == 1
            else:
                assert st.raw[at] == 0 and out.raw[96 * at:96 * at + 96] == oracle.g1_mul(oracle.g1_generator(), s)[1], (i, half)
