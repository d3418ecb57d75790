"""The shared-message entry points (nbls_verify_multiple_shared, nbls_verify_aggregates_shared, nbls_verify_aggregates_indexed_shared) without a GPU: exported by libnbls.so,
declared by the header (ABI 5), bound with their argument types, every refusal that needs no device work, group_messages, and the facade's exports and declarations."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
JS = os.path.join(PKG, 'js')
NAMES = ['nbls_verify_multiple_shared', 'nbls_verify_aggregates_shared', 'nbls_verify_aggregates_indexed_shared']
EINVAL = -1
DST = b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_'
# what the facade exported before the shared-message calls were added: they change how two of its functions work, not what it offers
FACADE_EXPORTS = ('CURVE,Fp,Fp12,Fp2,Fp6,Fr,PointG1,PointG2,aggregatePublicKeys,aggregateSignatures,getPublicKey,getPublicKeys,init,millerProduct,pairing,pairingBatch,sign,signBatch,'
                  'utils,verify,verifyBatch,verifyMultipleAggregateSignatures,verifyMultipleSignatures')


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
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    for nm in NAMES:
        assert 'int ' + nm + '(' in src, nm
    assert 'msg_index' in src and 'n_msgs' in src


def test_binding_argtypes(lib, pkg):
    bound = pkg.load_library()
    vp, sz, i32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_int)
    assert bound.nbls_verify_multiple_shared.argtypes == [vp, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp, i32p, vp]
    assert bound.nbls_verify_aggregates_shared.argtypes == [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, i32p, vp]
    assert bound.nbls_verify_aggregates_indexed_shared.argtypes == [vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, i32p, vp]
    for m in ('verify_multiple_shared', 'verify_aggregates_shared', 'verify_aggregates_indexed_shared'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.group_messages)


def test_refused_without_a_context(pkg):
    """a NULL context: NBLS_EINVAL from all three, whatever else is passed, and *all_ok untouched"""
    b = pkg.load_library()
    ok = C.c_int(7)
    sig, pk, msg = b'\xc0' + bytes(95), b'\xc0' + bytes(47), b'm'
    one, idx = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 1)(0)
    assert b.nbls_verify_multiple_shared(None, 1, sig, 1, msg, one, idx, pk, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert b.nbls_verify_aggregates_shared(None, 1, sig, 1, msg, one, idx, pk, one, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert b.nbls_verify_aggregates_indexed_shared(None, None, 1, sig, 1, msg, one, idx, idx, one, DST, len(DST), None, C.byref(ok), None) == EINVAL
    assert ok.value == 7


class FakeCtx(C.Structure):
    """Enough zeroed memory to stand for a context in calls that must be refused before they touch it beyond its mutex (a zeroed std::recursive_mutex is an unlocked one):
    every call below has to return from its argument checks, before the first device call."""
    _fields_ = [('raw', C.c_uint8 * (1 << 16))]


def test_refusals_before_any_device_work(pkg):
    """missing pointers, n_msgs 0 or > n, an index out of range, a message that no set names, decreasing offsets: NBLS_EINVAL, no GPU needed"""
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    ok = C.c_int(7)
    n = 4
    sigs, pks, msgs = (b'\xc0' + bytes(95)) * n, (b'\xc0' + bytes(47)) * n, b'aabbcc'
    seed = bytes(32)
    offs2 = (C.c_uint32 * 3)(0, 2, 4)
    koffs = (C.c_uint32 * 5)(0, 1, 2, 3, 4)
    good = (C.c_uint32 * n)(0, 1, 1, 0)

    def multiple(n_=n, sigs_=sigs, m_=2, msgs_=msgs, offs_=offs2, idx_=good, pks_=pks, dst_=DST, ok_=C.byref(ok)):
        return b.nbls_verify_multiple_shared(ctx, n_, sigs_, m_, msgs_, offs_, idx_, pks_, dst_, len(DST), seed, ok_, None)

    def aggregates(m_=2, offs_=offs2, idx_=good, koffs_=koffs, pks_=pks):
        return b.nbls_verify_aggregates_shared(ctx, n, sigs, m_, msgs, offs_, idx_, pks_, koffs_, DST, len(DST), seed, C.byref(ok), None)

    # missing pointers and sizes
    assert multiple(n_=0) == EINVAL
    assert multiple(sigs_=None) == EINVAL
    assert multiple(offs_=None) == EINVAL
    assert multiple(idx_=None) == EINVAL
    assert multiple(pks_=None) == EINVAL
    assert multiple(dst_=None) == EINVAL
    assert multiple(ok_=None) == EINVAL
    assert multiple(msgs_=None) == EINVAL          # no message bytes, but the offsets say there are some
    assert aggregates(koffs_=None) == EINVAL
    assert aggregates(pks_=None) == EINVAL
    # n_msgs
    assert multiple(m_=0) == EINVAL
    assert multiple(m_=n + 1, offs_=(C.c_uint32 * 6)(0, 1, 2, 3, 4, 5)) == EINVAL
    assert aggregates(m_=0) == EINVAL
    assert aggregates(m_=n + 1, offs_=(C.c_uint32 * 6)(0, 1, 2, 3, 4, 5)) == EINVAL
    # the index: out of range, a message that no set names
    for bad in ((0, 1, 2, 0), (0, 1, 0xffffffff, 0), (0, 0, 0, 0), (1, 1, 1, 1)):
        assert multiple(idx_=(C.c_uint32 * n)(*bad)) == EINVAL, bad
        assert aggregates(idx_=(C.c_uint32 * n)(*bad)) == EINVAL, bad
    assert multiple(m_=3, offs_=(C.c_uint32 * 4)(0, 2, 4, 6), idx_=(C.c_uint32 * n)(0, 2, 2, 0)) == EINVAL     # message 1 unreferenced
    # decreasing message offsets; the aggregate forms' key offsets (an empty set, decreasing)
    assert multiple(offs_=(C.c_uint32 * 3)(0, 4, 2)) == EINVAL
    assert aggregates(offs_=(C.c_uint32 * 3)(0, 4, 2)) == EINVAL
    assert aggregates(koffs_=(C.c_uint32 * 5)(0, 1, 1, 3, 4)) == EINVAL
    assert aggregates(koffs_=(C.c_uint32 * 5)(0, 2, 1, 3, 4)) == EINVAL
    # the indexed form: no table
    kidx = (C.c_uint32 * n)(0, 1, 2, 3)
    assert b.nbls_verify_aggregates_indexed_shared(ctx, None, n, sigs, 2, msgs, offs2, good, kidx, koffs, DST, len(DST), seed, C.byref(ok), None) == EINVAL
    assert ok.value == 7


def test_group_messages(pkg):
    g = pkg.group_messages
    assert g([]) == ([], [])
    assert g([b'a']) == ([b'a'], [0])
    assert g([b'a', b'a', b'a']) == ([b'a'], [0, 0, 0])
    assert g([b'b', b'a', b'b', b'', b'a', b'', b'c']) == ([b'b', b'a', b'', b'c'], [0, 1, 0, 2, 1, 2, 3])
    assert g([b'', b'']) == ([b''], [0, 0])
    assert g([b'ab', b'a', b'b', b'ab']) == ([b'ab', b'a', b'b'], [0, 1, 2, 0])          # byte equality of whole messages, not of their concatenation
    assert g([bytearray(b'x'), memoryview(b'x'), b'x']) == ([b'x'], [0, 0, 0])
    msgs = [b'root %d' % (i * 7 % 5) for i in range(100)]
    distinct, index = g(msgs)
    assert len(distinct) == 5 and [distinct[k] for k in index] == msgs and sorted(set(index)) == list(range(5))
    assert [index.index(k) for k in range(5)] == sorted(index.index(k) for k in range(5))   # first-appearance order


@pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')
def test_facade_exports_unchanged_and_native_calls_declared(lib):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    now = subprocess.check_output(['node', '-e', "const b=require('%s'); console.log(Object.keys(b).sort().join(','))" % os.path.join(JS, 'index.js')]).decode().strip()
    assert now == FACADE_EXPORTS
    dts = open(os.path.join(JS, 'index.d.ts')).read()
    assert 'verifyMultipleSharedAsync' in dts and 'verifyAggregatesSharedAsync' in dts
    napi = open(os.path.join(JS, 'nbls_napi.c')).read()
    assert 'verifyMultipleSharedAsync' in napi and 'verifyAggregatesSharedAsync' in napi
