"""The commitment-evaluation entry points (nbls_g1_poly_eval, nbls_g2_poly_eval) without a GPU: exported by libnbls.so, declared by the header (ABI 5), bound with their
argument types, every refusal that needs no device work, and the facade's statics and unchanged exports."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import pytest
import vmsim_py
from test_verify_shared_abi import FACADE_EXPORTS, FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
JS = os.path.join(PKG, 'js')
NAMES = ['nbls_g1_poly_eval', 'nbls_g2_poly_eval']
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
    for nm in NAMES + ['nbls_extra_program_kernel']:
        assert nm in exported, nm
        assert hasattr(lib, nm)
    for nm in ('nbls_poly_group_launch', 'nbls_poly_coef_launch', 'nbls_poly_status_launch', 'nbls_aot_extra_index'):          # the kernels' launch wrappers stay internal
        assert nm not in exported, nm
    assert not any('nbls_sim_' in nm for nm in exported)          # the simulator's entries for the programs are not in the product
    assert lib.nbls_abi_version() == 5
    assert lib.nbls_program_count() == len(vmsim_py.PROGS) + 1          # the numbered registry did not grow (tests/test_verify_multiple_sim.py pins the same count)


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    for nm in NAMES:
        assert 'int ' + nm + '(' in src, nm
    assert 'const char* nbls_extra_program_kernel(' in src
    assert '#define NBLS_TUNE_POLY_SLAB 15 ' in src
    flat = ' '.join(src.replace('*', ' ').split())
    assert 'nbls_g1_poly_eval, nbls_g2_poly_eval, nbls_extra_program_kernel, NBLS_TUNE_POLY_SLAB, scratch slots 57 .. 61 (additions only, same version)' in flat
    decl = flat[flat.index('Share public keys'):flat.index('int nbls_g1_poly_eval(')]
    assert 'NOT an interface for secrets' in decl and 'coef_offsets' in decl and 'id_offsets' in decl and 'LOWEST degree first' in decl


def test_binding_argtypes(lib, pkg):
    bound = pkg.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert bound.nbls_g1_poly_eval.argtypes == [vp, sz, vp, vp, vp, vp, vp, vp]
    assert bound.nbls_g2_poly_eval.argtypes == [vp, sz, vp, vp, vp, vp, vp, vp]
    assert bound.nbls_extra_program_kernel.argtypes == [vp, C.c_char_p] and bound.nbls_extra_program_kernel.restype == C.c_char_p
    for m in ('poly_eval', 'set_poly_slab', 'extra_program_kernel'):
        assert callable(getattr(pkg.Engine, m, None)), m


def test_refused_without_a_context(pkg):
    b = pkg.load_library()
    one = (C.c_uint32 * 2)(0, 1)
    x, out = (1).to_bytes(32, 'big'), C.create_string_buffer(96)
    assert b.nbls_g1_poly_eval(None, 1, one, b'\xc0' + bytes(47), one, x, out, None) == EINVAL
    assert b.nbls_g2_poly_eval(None, 1, one, b'\xc0' + bytes(95), one, x, out, None) == EINVAL
    assert b.nbls_extra_program_kernel(None, b'poly_g1_16') is None
    assert b.nbls_set_tuning(None, 15, 16) == EINVAL
    assert out.raw == bytes(96)


def test_refusals_before_any_device_work(pkg):
    """a missing pointer, n_groups = 0, offsets that do not strictly increase, more than 2^16 coefficients in a group, more than 2^24 coefficients or 2^22 identifiers in the
    call: NBLS_EINVAL, no GPU needed"""
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    ids = b''.join(i.to_bytes(32, 'big') for i in range(1, 7))
    out, st = C.create_string_buffer(96 * 6), C.create_string_buffer(6)
    good = (C.c_uint32 * 3)(0, 2, 6)
    for f, e in ((b.nbls_g1_poly_eval, 48), (b.nbls_g2_poly_eval, 96)):
        coefs = (b'\xc0' + bytes(e - 1)) * 6

        def call(m_=2, coff_=good, coefs_=coefs, ioff_=good, ids_=ids, out_=out):
            return f(ctx, m_, coff_, coefs_, ioff_, ids_, out_, st)

        assert call(m_=0) == EINVAL
        for k in ('coff_', 'coefs_', 'ioff_', 'ids_', 'out_'):
            assert call(**{k: None}) == EINVAL, k
        for k in ('coff_', 'ioff_'):
            assert call(**{k: (C.c_uint32 * 3)(0, 2, 2)}) == EINVAL          # an empty group
            assert call(**{k: (C.c_uint32 * 3)(0, 4, 2)}) == EINVAL          # decreasing
            assert call(**{k: (C.c_uint32 * 3)(2, 2, 6)}) == EINVAL
        assert call(coff_=(C.c_uint32 * 3)(0, 2, 2 + (1 << 16) + 1)) == EINVAL          # a polynomial of more than 2^16 coefficients
        assert call(coff_=(C.c_uint32 * 3)(5, 7, 7 + (1 << 16) + 1)) == EINVAL
        many = (C.c_uint32 * 258)(*[k << 16 for k in range(258)])                        # 257 polynomials of 2^16: more than 2^24 coefficients
        small = (C.c_uint32 * 258)(*range(258))
        assert call(m_=257, coff_=many, ioff_=small) == EINVAL
        assert call(ioff_=(C.c_uint32 * 3)(0, 2, (1 << 22) + 1)) == EINVAL               # more than 2^22 identifiers
        assert call(ioff_=(C.c_uint32 * 3)(9, 11, 9 + (1 << 22) + 1)) == EINVAL
    # the tuning key refuses a negative slab and takes the others (0 = the default) without touching the device
    assert b.nbls_set_tuning(ctx, 15, -1) == EINVAL
    assert b.nbls_set_tuning(ctx, 15, 16) == 0 and b.nbls_set_tuning(ctx, 15, 0) == 0
    assert out.raw == bytes(96 * 6)


def test_engine_rejects_ragged_groups(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    for groups, g2 in (([([bytes(96)], [1])], False), ([([bytes(48)], [1])], True), ([([], [1])], False), ([([bytes(48)], [])], False)):
        with pytest.raises(pkg.NblsError):
            pkg.Engine.poly_eval(e, groups, g2=g2)


@pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')
def test_facade_statics_and_unchanged_exports(lib):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    script = ("const b=require('%s'); console.log(Object.keys(b).sort().join(',')); "
              "console.log(['evalCommitment','evalCommitmentBatch'].map(k=>typeof b.PointG1[k]+typeof b.PointG2[k]).join(','))") % os.path.join(JS, 'index.js')
    keys, statics = subprocess.check_output(['node', '-e', script]).decode().split()
    assert keys == FACADE_EXPORTS
    assert statics == 'functionfunction,functionfunction'
    dts = open(os.path.join(JS, 'index.d.ts')).read()
    napi = open(os.path.join(JS, 'nbls_napi.c')).read()
    assert 'polyEvalAsync' in dts and 'polyEvalAsync' in napi and '"polyEval"' in napi
    assert 'evalCommitment(' in dts and 'evalCommitmentBatch(' in dts
