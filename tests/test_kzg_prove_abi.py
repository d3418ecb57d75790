"""The KZG prover's entry points (nbls_kzg_setup_*, nbls_fr_quotient_roots, nbls_kzg_commit_blobs, nbls_kzg_compute_proofs, nbls_kzg_compute_blob_proofs) without a GPU: exported
by libnbls.so, declared by the header (ABI 5), bound with their argument types, and every refusal that needs no device work."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_kzg_setup_create', 'nbls_kzg_setup_destroy', 'nbls_kzg_setup_log2n', 'nbls_fr_quotient_roots', 'nbls_kzg_commit_blobs', 'nbls_kzg_compute_proofs',
         'nbls_kzg_compute_blob_proofs']
EINVAL = -1
ZERO48 = b'\xc0' + bytes(47)


class FakeSetup(C.Structure):
    """struct nbls_kzg_setup as nbls_internal.h lays it out: the argument checks read the device and the size, nothing else"""
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
    for nm in ('nbls_kzg_quotient_launch', 'nbls_kzg_canon_launch', 'nbls_kzg_prove_tail_launch', 'msm_rows_dev', 'msm_rows_dev_plan', 'blob_challenges', 'kzg_table', 'kzg_proof_tail'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers and the internal cores stay internal
    assert not any('nbls_sim_' in nm for nm in exported)
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_kzg_setup nbls_kzg_setup;' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('nbls_kzg_setup_create / _destroy / _log2n, nbls_fr_quotient_roots, nbls_kzg_commit_blobs, nbls_kzg_compute_proofs, nbls_kzg_compute_blob_proofs, '
            'scratch slots 69 .. 70 (additions only, same version)') in flat
    decl = flat[flat.index("KZG, the prover's side"):flat.index('int nbls_kzg_compute_blob_proofs(')]
    for words in ('BIT-REVERSED ORDER', 'subgroup check included', 'NBLS_EDECODE', 'compute_quotient_eval_within_domain', 'ONLY HASHED, NOT DECODED', 'ZERO POINTS ARE VALID',
                  'ALL-ZERO bytes', 'NOT an interface for secrets', 'a setup created on another device', 'above 2^22'):
        assert words in decl, words
    assert 'is nbls_g1_msm_rows over the Lagrange basis' not in flat          # the sentence the prover's calls replace


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_kzg_setup_create.argtypes == [vp, u, vp, vp, C.POINTER(vp)]
    assert bound.nbls_kzg_setup_destroy.argtypes == [vp] and bound.nbls_kzg_setup_destroy.restype is None
    assert bound.nbls_kzg_setup_log2n.argtypes == [vp, C.POINTER(u)]
    assert bound.nbls_fr_quotient_roots.argtypes == [vp, u, sz, vp, vp, vp, vp, vp]
    assert bound.nbls_kzg_commit_blobs.argtypes == [vp, vp, sz, vp, vp, vp]
    assert bound.nbls_kzg_compute_proofs.argtypes == [vp, vp, sz, vp, vp, vp, vp, vp]
    assert bound.nbls_kzg_compute_blob_proofs.argtypes == [vp, vp, sz, vp, vp, vp, vp, vp]
    for m in ('kzg_setup', 'fr_quotient_roots', 'kzg_commit_blobs', 'kzg_compute_proofs', 'kzg_compute_blob_proofs'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.KzgSetup.close) and issubclass(pkg.KzgSetupError, pkg.NblsError)


def test_refused_without_a_context_or_a_setup(pkg):
    b = pkg.load_library()
    x = (1).to_bytes(32, 'big')
    out, y, q, h = C.create_string_buffer(48), C.create_string_buffer(32), C.create_string_buffer(128), C.c_void_p(7)
    su = C.byref(FakeSetup(0, 2, None))
    assert b.nbls_kzg_setup_create(None, 2, ZERO48 * 4, None, C.byref(h)) == EINVAL and h.value is None          # *out = NULL also on a refusal
    assert b.nbls_fr_quotient_roots(None, 2, 1, x * 4, x, y, q, None) == EINVAL
    assert b.nbls_fr_quotient_roots(None, 2, 0, None, None, None, None, None) == EINVAL          # a NULL context is refused even for an empty call
    assert b.nbls_kzg_commit_blobs(None, su, 1, x * 4, out, None) == EINVAL
    assert b.nbls_kzg_compute_proofs(None, su, 1, x * 4, x, out, y, None) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(None, su, 1, x * 4, ZERO48, None, out, None) == EINVAL
    ctx = C.byref(FakeCtx())
    assert b.nbls_kzg_commit_blobs(ctx, None, 1, x * 4, out, None) == EINVAL
    assert b.nbls_kzg_compute_proofs(ctx, None, 1, x * 4, x, out, y, None) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, None, 1, x * 4, ZERO48, None, out, None) == EINVAL
    k = C.c_uint(7)
    assert b.nbls_kzg_setup_log2n(None, C.byref(k)) == EINVAL and b.nbls_kzg_setup_log2n(su, None) == EINVAL
    assert b.nbls_kzg_setup_log2n(su, C.byref(k)) == 0 and k.value == 2
    b.nbls_kzg_setup_destroy(None)          # a no-op
    assert out.raw == bytes(48) and y.raw == bytes(32) and q.raw == bytes(128)


def test_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, cs, y, q, st, h = C.create_string_buffer(48), C.create_string_buffer(48), C.create_string_buffer(32), C.create_string_buffer(128), C.create_string_buffer(2), C.c_void_p(7)
    # nbls_kzg_setup_create: log2_n outside 1 .. 12, a missing pointer
    for k in (0, 13):
        h.value = 7
        assert b.nbls_kzg_setup_create(ctx, k, ZERO48 * 4, st, C.byref(h)) == EINVAL and h.value is None, k
    assert b.nbls_kzg_setup_create(ctx, 2, None, st, C.byref(h)) == EINVAL
    assert b.nbls_kzg_setup_create(ctx, 2, ZERO48 * 4, st, None) == EINVAL
    # nbls_fr_quotient_roots: the rules of nbls_fr_eval_roots
    assert b.nbls_fr_quotient_roots(ctx, 0, 1, x, x, y, q, st) == EINVAL
    assert b.nbls_fr_quotient_roots(ctx, 13, 1, x, x, y, q, st) == EINVAL
    for k in range(4):
        args = [x * 4, x, y, q]
        args[k] = None
        assert b.nbls_fr_quotient_roots(ctx, 2, 1, *args, st) == EINVAL, k
    assert b.nbls_fr_quotient_roots(ctx, 12, 4097, x, x, y, q, st) == EINVAL
    assert b.nbls_fr_quotient_roots(ctx, 1, (1 << 23) + 1, x, x, y, q, st) == EINVAL
    assert b.nbls_fr_quotient_roots(ctx, 2, 0, None, None, None, None, None) == 0
    # the three prover calls: n = 0, a missing pointer, a setup of another device, more than 2^22 scalars (1024 mainnet blobs fit exactly: 1025 is the first refused n)
    su, su12, far = C.byref(FakeSetup(0, 2, None)), C.byref(FakeSetup(0, 12, None)), C.byref(FakeSetup(1, 2, None))
    assert b.nbls_kzg_commit_blobs(ctx, su, 0, x * 4, out, st) == EINVAL
    assert b.nbls_kzg_commit_blobs(ctx, su, 1, None, out, st) == EINVAL
    assert b.nbls_kzg_commit_blobs(ctx, su, 1, x * 4, None, st) == EINVAL
    assert b.nbls_kzg_commit_blobs(ctx, far, 1, x * 4, out, st) == EINVAL
    assert b.nbls_kzg_commit_blobs(ctx, su12, 1025, x * 4, out, st) == EINVAL
    assert b.nbls_kzg_commit_blobs(ctx, su, (1 << 20) + 1, x * 4, out, st) == EINVAL
    assert b.nbls_kzg_compute_proofs(ctx, su, 0, x * 4, x, out, y, st) == EINVAL
    for k in range(4):
        args = [x * 4, x, out, y]
        args[k] = None
        assert b.nbls_kzg_compute_proofs(ctx, su, 1, *args, st) == EINVAL, k
    assert b.nbls_kzg_compute_proofs(ctx, far, 1, x * 4, x, out, y, st) == EINVAL
    assert b.nbls_kzg_compute_proofs(ctx, su12, 1025, x * 4, x, out, y, st) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, su, 0, x * 4, ZERO48, cs, out, st) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, su, 1, None, ZERO48, cs, out, st) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, su, 1, x * 4, ZERO48, cs, None, st) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, su, 1, x * 4, None, None, out, st) == EINVAL          # no commitments given: the place for the computed ones is required
    assert b.nbls_kzg_compute_blob_proofs(ctx, far, 1, x * 4, ZERO48, cs, out, st) == EINVAL
    assert b.nbls_kzg_compute_blob_proofs(ctx, su12, 1025, x * 4, ZERO48, cs, out, st) == EINVAL
    assert out.raw == bytes(48) and cs.raw == bytes(48) and y.raw == bytes(32) and q.raw == bytes(128) and st.raw == bytes(2)


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    su = pkg.KzgSetup(pkg.load_library(), C.byref(FakeSetup(0, 2, None)))
    su.close = lambda: None          # (not a handle the library made)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_setup(e, 2, [ZERO48] * 3)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_setup(e, 13, bytes(48 << 13))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_quotient_roots(e, 2, [[1, 2, 3]], [5])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_commit_blobs(e, su, [bytes(127)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_commit_blobs(e, su, [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_proofs(e, su, [bytes(128)], [1, 2])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_blob_proofs(e, su, [bytes(128)], [bytes(47)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_blob_proofs(e, su, [bytes(128), bytes(128)], [ZERO48])
    closed = pkg.KzgSetup(pkg.load_library(), None)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_commit_blobs(e, closed, [bytes(128)])
    su.h = None
