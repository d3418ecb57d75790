"""The PeerDAS entry points (nbls_fr_ntt, nbls_kzg_compute_cells, nbls_kzg_monomial_*, nbls_kzg_compute_cells_and_proofs, NBLS_TUNE_CELLS_CHUNK) without a GPU: exported by
libnbls.so, declared by the header (ABI 5), bound with their argument types, and every refusal that needs no device work."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_fr_ntt', 'nbls_kzg_compute_cells', 'nbls_kzg_monomial_create', 'nbls_kzg_monomial_destroy', 'nbls_kzg_monomial_log2n', 'nbls_kzg_compute_cells_and_proofs']
EINVAL = -1
ZERO48 = b'\xc0' + bytes(47)


class FakeMonomial(C.Structure):
    """struct nbls_kzg_monomial as nbls_internal.h lays it out: the argument checks read the device and the size, nothing else"""
    _fields_ = [('device', C.c_int), ('log2_n', C.c_uint), ('pts', C.c_void_p)]


@pytest.fixture(scope='module')
def lib():
    subprocess.check_call(['make', '-s', '-C', os.path.join(PKG, 'csrc'), '../libnbls.so'])
    return C.CDLL(os.path.join(PKG, 'libnbls.so'))


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


def test_symbols_exported(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls.so')]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for nm in NAMES:
        assert nm in exported, nm
        assert hasattr(lib, nm)
    for nm in ('nbls_kzg_ntt_launch', 'nbls_kzg_cell_rows_launch', 'nbls_kzg_inv_roots_launch', 'kzg_table', 'kzg_basis_create', 'kzg_basis_decode', 'kzg_basis_destroy', 'kzg_basis_log2n',
               'kzg_proof_tail', 'cells_pipeline'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers and the internal cores stay internal
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_kzg_monomial nbls_kzg_monomial;' in src
    assert '#define NBLS_NTT_TO_COEFFS 0' in src and '#define NBLS_NTT_TO_EVALS 1' in src and '#define NBLS_TUNE_CELLS_CHUNK 20' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('nbls_fr_ntt, NBLS_NTT_ , nbls_kzg_compute_cells, nbls_kzg_monomial_create / _destroy / _log2n, nbls_kzg_compute_cells_and_proofs, NBLS_TUNE_CELLS_CHUNK, '
            'scratch slots 71 .. 73 (additions only, same version)') in flat
    decl = flat[flat.index('PeerDAS (EIP-7594'):flat.index('int nbls_kzg_compute_cells_and_proofs(')]
    for words in ('bit-reversed order', 'NATURAL order', 'no permutation pass', '5 when the shift is 0 mod r', 'coset_for_cell', 'NBLS_EDECODE', 'ZERO POINTS ARE VALID',
                  'NOT an interface for secrets', 'a basis created on another device', '(2 N / c) N > 2^22', 'test vectors have not been run', 'No FK20'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_fr_ntt.argtypes == [vp, u, C.c_int, sz, vp, vp, vp, vp]
    assert bound.nbls_kzg_compute_cells.argtypes == [vp, u, u, sz, vp, vp, vp]
    assert bound.nbls_kzg_monomial_create.argtypes == [vp, u, vp, vp, C.POINTER(vp)]
    assert bound.nbls_kzg_monomial_destroy.argtypes == [vp] and bound.nbls_kzg_monomial_destroy.restype is None
    assert bound.nbls_kzg_monomial_log2n.argtypes == [vp, C.POINTER(u)]
    assert bound.nbls_kzg_compute_cells_and_proofs.argtypes == [vp, vp, u, sz, vp, vp, vp, vp]
    for m in ('fr_ntt', 'kzg_monomial_setup', 'kzg_compute_cells', 'kzg_compute_cells_and_proofs', 'set_cells_chunk'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.KzgMonomialSetup.close)


def test_refused_without_a_context_or_a_basis(pkg):
    b = pkg.load_library()
    x = (1).to_bytes(32, 'big')
    out, pf, h = C.create_string_buffer(256), C.create_string_buffer(48 * 8), C.c_void_p(7)
    mo = C.byref(FakeMonomial(0, 2, None))
    assert b.nbls_fr_ntt(None, 2, 0, 1, x * 4, None, out, None) == EINVAL
    assert b.nbls_fr_ntt(None, 2, 0, 0, None, None, None, None) == EINVAL          # a NULL context is refused even for an empty call
    assert b.nbls_kzg_compute_cells(None, 2, 1, 1, x * 4, out, None) == EINVAL
    assert b.nbls_kzg_compute_cells(None, 2, 1, 0, None, None, None) == EINVAL
    assert b.nbls_kzg_monomial_create(None, 2, ZERO48 * 4, None, C.byref(h)) == EINVAL and h.value is None          # *out = NULL also on a refusal
    assert b.nbls_kzg_compute_cells_and_proofs(None, mo, 1, 1, x * 4, out, pf, None) == EINVAL
    assert b.nbls_kzg_compute_cells_and_proofs(C.byref(FakeCtx()), None, 1, 1, x * 4, out, pf, None) == EINVAL
    assert b.nbls_set_tuning(None, 20, 1) == EINVAL
    k = C.c_uint(7)
    assert b.nbls_kzg_monomial_log2n(None, C.byref(k)) == EINVAL and b.nbls_kzg_monomial_log2n(mo, None) == EINVAL
    assert b.nbls_kzg_monomial_log2n(mo, C.byref(k)) == 0 and k.value == 2
    b.nbls_kzg_monomial_destroy(None)          # a no-op
    assert out.raw == bytes(256) and pf.raw == bytes(48 * 8)


def test_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, pf, st, h = C.create_string_buffer(256), C.create_string_buffer(48 * 8), C.create_string_buffer(2), C.c_void_p(7)
    # nbls_fr_ntt: the rules of nbls_fr_eval_roots, and the direction
    for k in (0, 13):
        assert b.nbls_fr_ntt(ctx, k, 0, 1, x * 4, None, out, st) == EINVAL, k
    for d in (-1, 2):
        assert b.nbls_fr_ntt(ctx, 2, d, 1, x * 4, None, out, st) == EINVAL, d
    assert b.nbls_fr_ntt(ctx, 2, 0, 1, None, x, out, st) == EINVAL
    assert b.nbls_fr_ntt(ctx, 2, 1, 1, x * 4, x, None, st) == EINVAL
    assert b.nbls_fr_ntt(ctx, 12, 0, 4097, x, None, out, st) == EINVAL
    assert b.nbls_fr_ntt(ctx, 1, 1, (1 << 23) + 1, x, None, out, st) == EINVAL
    for d in (0, 1):
        assert b.nbls_fr_ntt(ctx, 2, d, 0, None, None, None, None) == 0          # n = 0
    # nbls_kzg_compute_cells
    for k in (0, 13):
        assert b.nbls_kzg_compute_cells(ctx, k, 0, 1, x * 4, out, st) == EINVAL, k
    assert b.nbls_kzg_compute_cells(ctx, 2, 3, 1, x * 4, out, st) == EINVAL          # log2_cell > log2_n
    assert b.nbls_kzg_compute_cells(ctx, 2, 1, 1, None, out, st) == EINVAL
    assert b.nbls_kzg_compute_cells(ctx, 2, 1, 1, x * 4, None, st) == EINVAL
    assert b.nbls_kzg_compute_cells(ctx, 12, 6, 4097, x, out, st) == EINVAL
    assert b.nbls_kzg_compute_cells(ctx, 2, 1, 0, None, None, None) == 0
    # nbls_kzg_monomial_create: log2_n outside 1 .. 12, a missing pointer
    for k in (0, 13):
        h.value = 7
        assert b.nbls_kzg_monomial_create(ctx, k, ZERO48 * 4, st, C.byref(h)) == EINVAL and h.value is None, k
    assert b.nbls_kzg_monomial_create(ctx, 2, None, st, C.byref(h)) == EINVAL
    assert b.nbls_kzg_monomial_create(ctx, 2, ZERO48 * 4, st, None) == EINVAL
    # nbls_kzg_compute_cells_and_proofs: n = 0, a missing pointer, log2_cell > log2_n, a basis of another device, one blob above a pass of the batched MSM
    mo, mo12, mo11, far = (C.byref(FakeMonomial(0, 2, None)), C.byref(FakeMonomial(0, 12, None)), C.byref(FakeMonomial(0, 11, None)), C.byref(FakeMonomial(1, 2, None)))
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo, 1, 0, x * 4, out, pf, st) == EINVAL
    for k in range(3):
        args = [x * 4, out, pf]
        args[k] = None
        assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo, 1, 1, *args, st) == EINVAL, k
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo, 3, 1, x * 4, out, pf, st) == EINVAL
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, far, 1, 1, x * 4, out, pf, st) == EINVAL
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo12, 2, 1, x * 4, out, pf, st) == EINVAL          # 2^11 rows of 2^12 scalars = 2^23
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo11, 0, 1, x * 4, out, pf, st) == EINVAL          # 2^12 rows of 2^11 scalars = 2^23
    assert b.nbls_kzg_compute_cells_and_proofs(ctx, mo12, 6, 4097, x * 4, out, pf, st) == EINVAL          # more than 2^24 elements
    # the tuning key
    assert b.nbls_set_tuning(ctx, 20, -1) == EINVAL and b.nbls_set_tuning(ctx, 20, 2) == 0 and b.nbls_set_tuning(ctx, 20, 0) == 0 and b.nbls_set_tuning(ctx, 21, 0) == EINVAL
    assert out.raw == bytes(256) and pf.raw == bytes(48 * 8) and st.raw == bytes(2)


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    mo = pkg.KzgMonomialSetup(pkg.load_library(), C.byref(FakeMonomial(0, 2, None)))
    mo.close = lambda: None          # (not a handle the library made)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt(e, 2, [[1, 2, 3]], True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt(e, 2, [[1, 2, 3, 4]], False, [1, 2])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt(e, 13, bytes(32 << 13), True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_monomial_setup(e, 2, [ZERO48] * 3)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells(e, 2, 3, [bytes(128)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells(e, 2, 1, [bytes(127)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs(e, mo, 1, [bytes(127)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs(e, mo, 1, [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs(e, mo, 3, [bytes(128)])
    closed = pkg.KzgMonomialSetup(pkg.load_library(), None)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs(e, closed, 1, [bytes(128)])
    mo.h = None
