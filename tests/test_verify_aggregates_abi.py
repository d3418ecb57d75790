"""nbls_verify_aggregates without a GPU: the five entry points exported by libnbls.so, declared by the header (ABI 5) and bound with their argument types, the Engine methods,
the calls refused before any device work, and the facade's export."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
JS = os.path.join(PKG, 'js')
NAMES = ['nbls_verify_aggregates', 'nbls_verify_aggregates_indexed', 'nbls_keyset_create', 'nbls_keyset_destroy', 'nbls_keyset_size']
EINVAL = -1
DST = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'


@pytest.fixture(scope='module')
def lib():
    subprocess.check_call(['make', '-s', '-C', os.path.join(PKG, 'csrc'), '../libnbls.so'])
    return C.CDLL(os.path.join(PKG, 'libnbls.so'))


def test_symbols_exported(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls.so')]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for nm in NAMES:
        assert nm in exported, nm
        assert hasattr(lib, nm)
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_keyset nbls_keyset;' in src
    for nm in NAMES:
        assert nm + '(' in src, nm


def test_binding_argtypes(lib):
    pkg = importlib.import_module('noble-bls12-381_amd')
    bound = pkg.load_library()
    vp, sz, i32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_int)
    assert bound.nbls_verify_aggregates.argtypes == [vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, i32p, vp]
    assert bound.nbls_verify_aggregates_indexed.argtypes == [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, i32p, vp]
    assert bound.nbls_keyset_create.argtypes == [vp, sz, vp, vp, C.POINTER(vp)]
    assert bound.nbls_keyset_destroy.argtypes == [vp] and bound.nbls_keyset_destroy.restype is None
    assert bound.nbls_keyset_size.argtypes == [vp, C.POINTER(sz)]


def test_engine_methods():
    pkg = importlib.import_module('noble-bls12-381_amd')
    for m in ('verify_aggregates', 'verify_aggregates_indexed', 'create_keyset'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert hasattr(pkg, 'KeySet')


def test_refused_without_a_context(lib):
    """null context, null table, missing pointers: NBLS_EINVAL before any device work (no GPU needed)"""
    pkg = importlib.import_module('noble-bls12-381_amd')
    b = pkg.load_library()
    ok = C.c_int(7)
    sig, pk, msg = b'\xc0' + bytes(95), b'\xc0' + bytes(47), b'm'
    one = (C.c_uint32 * 2)(0, 1)
    empty = (C.c_uint32 * 2)(0, 0)
    for koffs in (one, empty):
        assert b.nbls_verify_aggregates(None, 1, sig, msg, one, pk, koffs, DST, len(DST), None, C.byref(ok), None) == EINVAL
        idx = (C.c_uint32 * 1)(0)
        assert b.nbls_verify_aggregates_indexed(None, None, 1, sig, msg, one, idx, koffs, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert ok.value == 7
    ks = C.c_void_p(1234)
    assert b.nbls_keyset_create(None, 1, pk, None, C.byref(ks)) == EINVAL
    n = C.c_size_t(99)
    assert b.nbls_keyset_size(None, C.byref(n)) == EINVAL and n.value == 99
    b.nbls_keyset_destroy(None)


@pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')
def test_facade_exports_verify_aggregates(lib):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    out = subprocess.check_output(['node', '-e', "const b=require('%s'); console.log(typeof b.verifyMultipleAggregateSignatures)" % os.path.join(JS, 'index.js')]).decode()
    assert out.strip() == 'function'
    dts = open(os.path.join(JS, 'index.d.ts')).read()
    assert 'verifyMultipleAggregateSignatures' in dts
