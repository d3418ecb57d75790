"""The KZG entry points (nbls_fr_eval_roots, nbls_kzg_verify_proofs, nbls_kzg_verify_blobs) without a GPU: exported by libnbls.so, declared by the header (ABI 5), bound with
their argument types, and every refusal that needs no device work."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_fr_eval_roots', 'nbls_kzg_verify_proofs', 'nbls_kzg_verify_blobs']
EINVAL = -1
ZERO48 = b'\xc0' + bytes(47)


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
    for nm in ('nbls_kzg_roots_launch', 'nbls_kzg_eval_launch', 'nbls_kzg_items_launch', 'nbls_agg_fix_zero_launch', 'nbls_kzg_item_scalars_launch', 'nbls_kzg_item_status_launch'):
        assert nm not in exported, nm          # the kernels' launch wrappers stay internal
    assert not any('nbls_sim_' in nm for nm in exported)
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert '#define NBLS_ST_NON_CANONICAL 21 ' in src
    for nm in NAMES:
        assert 'int ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert 'nbls_fr_eval_roots, nbls_kzg_verify_proofs, nbls_kzg_verify_blobs, NBLS_ST_NON_CANONICAL, scratch slots 64 .. 68 (additions only, same version)' in flat
    decl = flat[flat.index('KZG on BLS12-381'):flat.index('int nbls_kzg_verify_blobs(')]
    for words in ('bit-reversed order', 'ZERO POINTS ARE VALID', 'FSBLOBVERIFY_V1_', 'fast reject', 'NBLS_EDECODE', 'must be CANONICAL', 'n > 2^22', 'NOT written'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u, pi = C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_int32)
    assert bound.nbls_fr_eval_roots.argtypes == [vp, u, sz, vp, vp, vp, vp]
    assert bound.nbls_kzg_verify_proofs.argtypes == [vp, sz, vp, vp, vp, vp, vp, vp, pi, vp]
    assert bound.nbls_kzg_verify_blobs.argtypes == [vp, u, sz, vp, vp, vp, vp, vp, pi, vp]
    for m in ('fr_eval_roots', 'kzg_verify_proofs', 'kzg_verify_blobs'):
        assert callable(getattr(pkg.Engine, m, None)), m


def test_refused_without_a_context(pkg):
    b = pkg.load_library()
    ok, out = C.c_int32(7), C.create_string_buffer(32)
    x = (1).to_bytes(32, 'big')
    assert b.nbls_fr_eval_roots(None, 2, 1, x * 4, x, out, None) == EINVAL
    assert b.nbls_fr_eval_roots(None, 2, 0, None, None, None, None) == EINVAL          # a NULL context is refused even for an empty call
    assert b.nbls_kzg_verify_proofs(None, 1, ZERO48, x, x, ZERO48, bytes(96), None, C.byref(ok), None) == EINVAL
    assert b.nbls_kzg_verify_blobs(None, 2, 1, x * 4, ZERO48, ZERO48, bytes(96), None, C.byref(ok), None) == EINVAL
    assert ok.value == 7 and out.raw == bytes(32)


def test_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, st, ok = C.create_string_buffer(64), C.create_string_buffer(2), C.c_int32(7)
    # nbls_fr_eval_roots: log2_n outside 1 .. 12, missing buffers with n > 0, more than 2^24 elements; n = 0 is NBLS_OK
    assert b.nbls_fr_eval_roots(ctx, 0, 1, x, x, out, st) == EINVAL
    assert b.nbls_fr_eval_roots(ctx, 13, 1, x, x, out, st) == EINVAL
    for k in range(3):
        args = [x * 4, x, out]
        args[k] = None
        assert b.nbls_fr_eval_roots(ctx, 2, 1, *args, st) == EINVAL, k
    assert b.nbls_fr_eval_roots(ctx, 12, 4097, x, x, out, st) == EINVAL
    assert b.nbls_fr_eval_roots(ctx, 1, (1 << 23) + 1, x, x, out, st) == EINVAL
    assert b.nbls_fr_eval_roots(ctx, 2, 0, None, None, None, None) == 0
    # nbls_kzg_verify_proofs: n = 0, too many items, a missing pointer
    good = [ZERO48, x, x, ZERO48, bytes(96)]
    goodb = [x * 4, ZERO48, ZERO48, bytes(96)]
    assert b.nbls_kzg_verify_proofs(ctx, 0, *good, None, C.byref(ok), st) == EINVAL
    assert b.nbls_kzg_verify_proofs(ctx, (1 << 22) + 1, *good, None, C.byref(ok), st) == EINVAL          # 2^22 itself is inside the contract: the first refused n
    assert b.nbls_kzg_verify_blobs(ctx, 1, (1 << 22) + 1, *goodb, None, C.byref(ok), st) == EINVAL
    for k in range(5):
        args = list(good)
        args[k] = None
        assert b.nbls_kzg_verify_proofs(ctx, 1, *args, None, C.byref(ok), st) == EINVAL, k
    assert b.nbls_kzg_verify_proofs(ctx, 1, *good, None, None, st) == EINVAL
    # nbls_kzg_verify_blobs: the same, and log2_n
    assert b.nbls_kzg_verify_blobs(ctx, 2, 0, *goodb, None, C.byref(ok), st) == EINVAL
    assert b.nbls_kzg_verify_blobs(ctx, 0, 1, *goodb, None, C.byref(ok), st) == EINVAL
    assert b.nbls_kzg_verify_blobs(ctx, 13, 1, *goodb, None, C.byref(ok), st) == EINVAL
    assert b.nbls_kzg_verify_blobs(ctx, 12, 4097, *goodb, None, C.byref(ok), st) == EINVAL
    for k in range(4):
        args = list(goodb)
        args[k] = None
        assert b.nbls_kzg_verify_blobs(ctx, 2, 1, *args, None, C.byref(ok), st) == EINVAL, k
    assert b.nbls_kzg_verify_blobs(ctx, 2, 1, *goodb, None, None, st) == EINVAL
    assert ok.value == 7 and out.raw == bytes(64)


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_eval_roots(e, 2, [[1, 2, 3]], [5])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_verify_proofs(e, [ZERO48], [1], [1, 2], [ZERO48], bytes(96))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_verify_proofs(e, [ZERO48], [1], [1], [bytes(47)], bytes(96))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_verify_blobs(e, 2, [bytes(127)], [ZERO48], [ZERO48], bytes(96))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_verify_blobs(e, 2, [bytes(128)], [ZERO48], [ZERO48], bytes(95))
