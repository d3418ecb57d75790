"""The large transform's entry points (nbls_fr_ntt_large, nbls_fr_ntt_dev, NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS) without a GPU: exported by libnbls.so, declared by the
header (ABI 5), bound with their argument types, and every refusal that needs no device work.  nbls_fr_ntt keeps its own bound."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_fr_ntt_large', 'nbls_fr_ntt_dev']
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
    for nm in ('nbls_kzg_ntt_pass_launch', 'nbls_kzg_ntt_tail_launch', 'nbls_kzg_ntt_launch', 'fr_ntt_large_dev', 'ntt_large_args', 'kzg_table'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers and the internal core stay internal
    assert lib.nbls_abi_version() == 5
    sim = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls_sim.so')]).decode()
    assert 'nbls_sim_fr_ntt_large' in sim


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert '#define NBLS_TUNE_NTT_TAIL_BITS 26' in src and '#define NBLS_TUNE_NTT_PASS_BITS 27' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert 'Then nbls_fr_ntt_large, nbls_fr_ntt_dev, NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS, scratch slot 87 (additions only, same version).' in flat
    assert 'int nbls_fr_ntt(nbls_ctx ctx, unsigned log2_n / 1 .. 12 /' in flat          # the one-workgroup call keeps its bound
    decl = flat[flat.index('nbls_fr_ntt_large / nbls_fr_ntt_dev:'):flat.index('int nbls_fr_ntt_dev(')]
    for words in ('up to 2^24 elements', 'word for word', 'non-canonical before zero', 'the same bytes', 'no table of N roots exists', 'omega_N^rev_K(B)',
                  'the bytes never depend on them', 'K <= 12 is required', 'log2_n outside 1 .. 24', 'n = 0 is NBLS_OK', '16-byte aligned', 'd_out32 may equal d_in32',
                  'any other overlap is NBLS_EINVAL', 'asynchronous'):
        assert words in decl, words
    internal = open(os.path.join(PKG, 'csrc', 'nbls_internal.h')).read()
    assert 'SB_NTTL_FLAGS = 87,' in internal and 'static_assert(NSB == 88' in internal


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_fr_ntt_large.argtypes == [vp, u, C.c_int, sz, vp, vp, vp, vp]
    assert bound.nbls_fr_ntt_dev.argtypes == [vp, u, C.c_int, sz, vp, vp, vp, vp, vp]
    for m in ('fr_ntt_large', 'fr_ntt_dev', 'set_ntt_plan', 'fr_ntt'):
        assert callable(getattr(pkg.Engine, m, None)), m


def test_refused_without_a_context(pkg):
    b = pkg.load_library()
    x = (1).to_bytes(32, 'big')
    out = C.create_string_buffer(256)
    assert b.nbls_fr_ntt_large(None, 2, 0, 1, x * 4, None, out, None) == EINVAL
    assert b.nbls_fr_ntt_large(None, 2, 0, 0, None, None, None, None) == EINVAL          # a NULL context is refused even for an empty call
    assert b.nbls_fr_ntt_dev(None, 2, 0, 1, 4096, None, 8192, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(None, 2, 0, 0, None, None, None, None, None) == EINVAL
    assert b.nbls_set_tuning(None, 26, 1) == EINVAL and b.nbls_set_tuning(None, 27, 1) == EINVAL
    assert out.raw == bytes(256)


def test_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, st = C.create_string_buffer(256), C.create_string_buffer(2)
    for k in (0, 25, 32):
        assert b.nbls_fr_ntt_large(ctx, k, 0, 1, x * 4, None, out, st) == EINVAL, k
        assert b.nbls_fr_ntt_dev(ctx, k, 0, 1, 4096, None, 8192, None, None) == EINVAL, k
    for d in (-1, 2):
        assert b.nbls_fr_ntt_large(ctx, 2, d, 1, x * 4, None, out, st) == EINVAL, d
        assert b.nbls_fr_ntt_dev(ctx, 2, d, 1, 4096, None, 8192, None, None) == EINVAL, d
    assert b.nbls_fr_ntt_large(ctx, 2, 0, 1, None, x, out, st) == EINVAL
    assert b.nbls_fr_ntt_large(ctx, 2, 1, 1, x * 4, x, None, st) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 2, 0, 1, None, None, 8192, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 2, 0, 1, 4096, None, None, None, None) == EINVAL
    # more than 2^24 elements in the call
    assert b.nbls_fr_ntt_large(ctx, 12, 0, 4097, x, None, out, st) == EINVAL
    assert b.nbls_fr_ntt_large(ctx, 13, 0, 2049, x, None, out, st) == EINVAL
    assert b.nbls_fr_ntt_large(ctx, 24, 1, 2, x, None, out, st) == EINVAL
    assert b.nbls_fr_ntt_large(ctx, 1, 1, (1 << 23) + 1, x, None, out, st) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 24, 1, 2, 4096, None, 4096, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 14, 1, 1025, 4096, None, 4096, None, None) == EINVAL
    # the device-resident call: alignment and overlap (in place is allowed: it gets past these checks only with a real context)
    assert b.nbls_fr_ntt_dev(ctx, 13, 1, 1, 4096 + 8, None, 1 << 30, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 13, 1, 1, 4096, None, (1 << 30) + 4, None, None) == EINVAL
    row = 32 << 13
    assert b.nbls_fr_ntt_dev(ctx, 13, 1, 1, 1 << 30, None, (1 << 30) + row - 32, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 13, 1, 1, (1 << 30) + 16, None, 1 << 30, None, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 13, 0, 2, 1 << 30, None, (1 << 30) + row, None, None) == EINVAL
    for d in (0, 1):
        assert b.nbls_fr_ntt_large(ctx, 2, d, 0, None, None, None, None) == 0          # n = 0
        assert b.nbls_fr_ntt_large(ctx, 24, d, 0, None, None, None, None) == 0
        assert b.nbls_fr_ntt_dev(ctx, 20, d, 0, None, None, None, None, None) == 0
    assert out.raw == bytes(256) and st.raw == bytes(2)


def test_tuning_keys(pkg):
    b = pkg.load_library()
    fake = FakeCtx()
    ctx = C.byref(fake)
    x = (1).to_bytes(32, 'big')
    out = C.create_string_buffer(256)
    assert b.nbls_set_tuning(ctx, 25, 0) == EINVAL and b.nbls_set_tuning(ctx, 28, 0) == EINVAL          # the keys in front and behind stay unassigned
    for v in (0, 1, 12):
        assert b.nbls_set_tuning(ctx, 26, v) == 0, v
    for v in (-1, 13, 24):
        assert b.nbls_set_tuning(ctx, 26, v) == EINVAL, v
    for v in (0, 1, 9):
        assert b.nbls_set_tuning(ctx, 27, v) == 0, v
    for v in (-1, 10):
        assert b.nbls_set_tuning(ctx, 27, v) == EINVAL, v
    # a tail size that leaves more than 12 global stages is refused before any device work
    assert b.nbls_set_tuning(ctx, 26, 1) == 0
    assert b.nbls_fr_ntt_large(ctx, 14, 1, 1, x, None, out, None) == EINVAL
    assert b.nbls_fr_ntt_dev(ctx, 14, 1, 1, 4096, None, 4096, None, None) == EINVAL
    assert b.nbls_set_tuning(ctx, 26, 0) == 0 and b.nbls_set_tuning(ctx, 27, 0) == 0
    assert bytes(fake.raw) == bytes(1 << 16)          # both keys back at their defaults: nothing else of the context was written


def test_the_one_workgroup_call_keeps_its_bound(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, st = C.create_string_buffer(256), C.create_string_buffer(2)
    assert b.nbls_fr_ntt(ctx, 13, 0, 1, x * 4, None, out, st) == EINVAL
    assert b.nbls_fr_ntt(ctx, 13, 1, 1, x * 4, None, out, st) == EINVAL
    assert b.nbls_fr_eval_roots(ctx, 13, 1, x * 4, x, out, st) == EINVAL


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt_large(e, 2, [[1, 2, 3]], True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt_large(e, 2, [[1, 2, 3, 4]], False, [1, 2])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt_large(e, 25, bytes(64), True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt_large(e, 13, bytes((32 << 13) - 32), True)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.fr_ntt_large(e, 13, bytes(32 << 13), True, bytes(64))
