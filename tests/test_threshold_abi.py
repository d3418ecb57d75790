"""The Fr and threshold-recombination entry points (nbls_fr_op_batch, nbls_lagrange_at_zero, nbls_g2_combine_shares, nbls_g1_combine_shares) without a GPU: exported by
libnbls.so, declared by the header (ABI 5), bound with their argument types, every refusal that needs no device work, and the facade's statics and unchanged exports."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import pytest
from test_verify_shared_abi import FACADE_EXPORTS, FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
JS = os.path.join(PKG, 'js')
NAMES = ['nbls_fr_op_batch', 'nbls_lagrange_at_zero', 'nbls_g2_combine_shares', 'nbls_g1_combine_shares']
EINVAL = -1


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
    assert 'nbls_fr_lagrange_launch' not in exported          # the kernels' launch wrappers stay internal
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    for nm in NAMES:
        assert 'int ' + nm + '(' in src, nm
    for i, nm in enumerate(('ADD', 'SUB', 'NEG', 'MUL', 'SQR', 'INV', 'DIV', 'POW')):
        assert '#define NBLS_FROP_%s %d\n' % (nm, i) in src
    assert '#define NBLS_ST_BAD_IDS 20\n' in src
    assert 'group_offsets' in src and 'ids32' in src
    assert 'not an interface for secrets' in ' '.join(src.lower().replace('*', ' ').split())          # the Fr calls wipe nothing: said where they are declared


def test_binding_argtypes(lib, pkg):
    bound = pkg.load_library()
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    assert bound.nbls_fr_op_batch.argtypes == [vp, i32, sz, vp, vp, vp, vp]
    assert bound.nbls_lagrange_at_zero.argtypes == [vp, sz, vp, vp, vp, vp]
    assert bound.nbls_g2_combine_shares.argtypes == [vp, sz, vp, vp, vp, vp, vp]
    assert bound.nbls_g1_combine_shares.argtypes == [vp, sz, vp, vp, vp, vp, vp]
    for m in ('fr_op', 'lagrange_at_zero', 'combine_shares'):
        assert callable(getattr(pkg.Engine, m, None)), m


def test_refused_without_a_context(pkg):
    b = pkg.load_library()
    one = (C.c_uint32 * 2)(0, 1)
    x, out = (1).to_bytes(32, 'big'), C.create_string_buffer(96)
    assert b.nbls_fr_op_batch(None, 0, 1, x, x, out, None) == EINVAL
    assert b.nbls_lagrange_at_zero(None, 1, one, x, out, None) == EINVAL
    assert b.nbls_g2_combine_shares(None, 1, one, x, b'\xc0' + bytes(95), out, None) == EINVAL
    assert b.nbls_g1_combine_shares(None, 1, one, x, b'\xc0' + bytes(47), out, None) == EINVAL
    assert out.raw == bytes(96)


def test_refusals_before_any_device_work(pkg):
    """a missing pointer, n_groups = 0, offsets that do not strictly increase, more than 2^24 shares, a group of more than 2^16: NBLS_EINVAL, no GPU needed"""
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    n = 6
    ids = b''.join(i.to_bytes(32, 'big') for i in range(1, n + 1))
    sig, pk = (b'\xc0' + bytes(95)) * n, (b'\xc0' + bytes(47)) * n
    out, st = C.create_string_buffer(96 * n), C.create_string_buffer(n)
    good = (C.c_uint32 * 3)(0, 2, 6)

    def lag(m_=2, offs_=good, ids_=ids, out_=out):
        return b.nbls_lagrange_at_zero(ctx, m_, offs_, ids_, out_, st)

    def g2(m_=2, offs_=good, ids_=ids, sh_=sig, out_=out):
        return b.nbls_g2_combine_shares(ctx, m_, offs_, ids_, sh_, out_, st)

    def g1(m_=2, offs_=good, ids_=ids, sh_=pk, out_=out):
        return b.nbls_g1_combine_shares(ctx, m_, offs_, ids_, sh_, out_, st)

    for f in (lag, g2, g1):
        assert f(m_=0) == EINVAL
        assert f(offs_=None) == EINVAL
        assert f(ids_=None) == EINVAL
        assert f(out_=None) == EINVAL
        assert f(offs_=(C.c_uint32 * 3)(0, 2, 2)) == EINVAL          # an empty group
        assert f(offs_=(C.c_uint32 * 3)(0, 4, 2)) == EINVAL          # decreasing
        assert f(offs_=(C.c_uint32 * 3)(2, 2, 6)) == EINVAL
        assert f(offs_=(C.c_uint32 * 3)(0, 2, 2 + (1 << 16) + 1)) == EINVAL          # a group of more than 2^16 shares
        assert f(offs_=(C.c_uint32 * 3)(5, 7, 7 + (1 << 16) + 1)) == EINVAL
        many = (C.c_uint32 * 258)(*[k << 16 for k in range(258)])                      # 257 groups of 2^16: more than 2^24 shares
        assert f(m_=257, offs_=many) == EINVAL
    assert g2(sh_=None) == EINVAL
    assert g1(sh_=None) == EINVAL
    # nbls_fr_op_batch: a missing pointer, an unknown operation, a binary operation without its second operand
    x = ids[:64]
    fr = lambda op, n_=2, a_=x, b_=x, out_=out: b.nbls_fr_op_batch(ctx, op, n_, a_, b_, out_, st)
    assert fr(-1) == EINVAL and fr(8) == EINVAL
    assert fr(0, a_=None) == EINVAL and fr(0, out_=None) == EINVAL
    for op in (0, 1, 3, 6, 7):
        assert fr(op, b_=None) == EINVAL
    assert fr(3, n_=(1 << 24) + 1) == EINVAL
    assert out.raw == bytes(96 * n)


def test_engine_rejects_ragged_groups(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    with pytest.raises(pkg.NblsError):
        pkg.Engine.combine_shares(e, [([1, 2], [bytes(96)])])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.combine_shares(e, [([1], [bytes(48)])], g2=True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_op(e, 'add', [1, 2], [3])
    assert pkg.Engine._fr32(5) == (5).to_bytes(32, 'big') and pkg.Engine._fr32(bytearray(32)) == bytes(32)
    with pytest.raises(pkg.NblsError):
        pkg.Engine._fr32(bytes(31))


@pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')
def test_facade_statics_and_unchanged_exports(lib):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    script = ("const b=require('%s'); console.log(Object.keys(b).sort().join(',')); "
              "console.log(['combineShares','combineSharesBatch'].map(k=>typeof b.PointG1[k]+typeof b.PointG2[k]).join(','))") % os.path.join(JS, 'index.js')
    keys, statics = subprocess.check_output(['node', '-e', script]).decode().split()
    assert keys == FACADE_EXPORTS
    assert statics == 'functionfunction,functionfunction'
    dts = open(os.path.join(JS, 'index.d.ts')).read()
    napi = open(os.path.join(JS, 'nbls_napi.c')).read()
    for nm in ('combineSharesAsync', 'lagrangeAtZeroAsync', 'frOpAsync'):
        assert nm in dts and nm in napi, nm
    assert 'combineShares(' in dts and 'combineSharesBatch(' in dts
