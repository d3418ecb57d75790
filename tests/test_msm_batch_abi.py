"""The batched multi-scalar multiplication (nbls_g*_msm_batch, nbls_g*_msm_rows) without a GPU: exported by libnbls.so, declared by the header (ABI 5), bound with their
argument types, and every refusal that needs no device work."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
import vmsim_py
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_g1_msm_batch', 'nbls_g2_msm_batch', 'nbls_g1_msm_rows', 'nbls_g2_msm_rows']
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
        assert nm in exported and hasattr(lib, nm), nm
    for nm in ('nbls_msm_keys_launch', 'nbls_msm_bitsel_launch'):            # the kernels' launch wrappers stay internal
        assert nm not in exported, nm
    assert lib.nbls_abi_version() == 5
    assert lib.nbls_program_count() == len(vmsim_py.PROGS) + 1          # the numbered registry did not grow


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    for nm in NAMES:
        assert 'int ' + nm + '(' in src, nm
    assert '#define NBLS_TUNE_MSMB_WINDOW 16 ' in src and '#define NBLS_TUNE_MSMB_BIG 17 ' in src and '#define NBLS_TUNE_MSMB_SLAB 18 ' in src
    flat = ' '.join(src.replace('*', ' ').split())
    assert 'nbls_g1_msm_rows, nbls_g2_msm_rows, NBLS_TUNE_MSMB_WINDOW / _BIG / _SLAB' in flat and 'scratch slots 62 .. 63 (additions only, same version)' in flat
    decl = flat[flat.index('Many independent sums in one call'):flat.index('int nbls_g1_msm_batch(')]
    for words in ('NON-DECREASING', 'byte for byte', 'not an interface for secrets', 'n_pts = 0', 'more than 2^22 points or scalars', 'than 2^20 groups or rows'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert bound.nbls_g1_msm_batch.argtypes == [vp, sz, vp, vp, vp, vp, vp] and bound.nbls_g2_msm_batch.argtypes == [vp, sz, vp, vp, vp, vp, vp]
    assert bound.nbls_g1_msm_rows.argtypes == [vp, sz, vp, sz, vp, vp, vp] and bound.nbls_g2_msm_rows.argtypes == [vp, sz, vp, sz, vp, vp, vp]
    for m in ('msm_batch', 'msm_rows', 'set_msm_batch'):
        assert callable(getattr(pkg.Engine, m, None)), m


def test_refusals_before_any_device_work(pkg):
    """without a context; then on zeroed memory that stands for one: a missing pointer, no group / row / point, decreasing offsets, more than 2^22 points or scalars, more than
    2^20 groups or rows -- NBLS_EINVAL, no GPU needed, nothing written"""
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    K = bytes(32 * 4)
    out, st = C.create_string_buffer(192 * 4), C.create_string_buffer(4)
    offs = (C.c_uint32 * 3)(0, 2, 4)
    for f, sz in ((b.nbls_g1_msm_batch, 96), (b.nbls_g2_msm_batch, 192)):
        P = bytes(sz * 4)
        assert f(None, 2, offs, P, K, out, st) == EINVAL
        assert f(ctx, 2, None, P, K, out, st) == EINVAL and f(ctx, 2, offs, None, K, out, st) == EINVAL and f(ctx, 2, offs, P, None, out, st) == EINVAL
        assert f(ctx, 2, offs, P, K, None, st) == EINVAL
        assert f(ctx, 0, offs, P, K, out, st) == EINVAL
        assert f(ctx, 2, (C.c_uint32 * 3)(0, 3, 2), P, K, out, st) == EINVAL and f(ctx, 2, (C.c_uint32 * 3)(3, 2, 4), P, K, out, st) == EINVAL
        assert f(ctx, 1, (C.c_uint32 * 2)(0, (1 << 22) + 1), P, K, out, st) == EINVAL and f(ctx, 1, (C.c_uint32 * 2)(7, 7 + (1 << 22) + 1), P, K, out, st) == EINVAL
        assert f(ctx, (1 << 20) + 1, offs, P, K, out, st) == EINVAL
    for f, sz in ((b.nbls_g1_msm_rows, 96), (b.nbls_g2_msm_rows, 192)):
        P = bytes(sz * 4)
        assert f(None, 2, P, 2, K, out, st) == EINVAL
        assert f(ctx, 2, None, 2, K, out, st) == EINVAL and f(ctx, 2, P, 2, None, out, st) == EINVAL and f(ctx, 2, P, 2, K, None, st) == EINVAL
        assert f(ctx, 2, P, 0, K, out, st) == EINVAL and f(ctx, 0, P, 2, K, out, st) == EINVAL and f(ctx, 0, P, 0, K, out, st) == EINVAL
        assert f(ctx, (1 << 22) + 1, P, 1, K, out, st) == EINVAL and f(ctx, 1 << 11, P, (1 << 11) + 1, K, out, st) == EINVAL
        assert f(ctx, 1, P, (1 << 20) + 1, K, out, st) == EINVAL
    assert out.raw == bytes(192 * 4) and st.raw == bytes(4)
    # the tuning keys: the window takes 0 and the five widths, the others anything that is not negative (0 = the default), without touching the device
    assert b.nbls_set_tuning(None, 16, 8) == EINVAL
    for w in (0, 4, 6, 8, 10, 12):
        assert b.nbls_set_tuning(ctx, 16, w) == 0, w
    for w in (-4, 1, 2, 5, 7, 14, 16):
        assert b.nbls_set_tuning(ctx, 16, w) == EINVAL, w
    for key in (17, 18):
        assert b.nbls_set_tuning(ctx, key, -1) == EINVAL and b.nbls_set_tuning(ctx, key, 64) == 0 and b.nbls_set_tuning(ctx, key, 0) == 0
    assert b.nbls_set_tuning(ctx, 19, 0) == EINVAL


def test_engine_rejects_ragged_input(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    with pytest.raises(AssertionError):
        pkg.Engine.msm_batch(e, [bytes(96)], [[bytes(32)] * 2])
    with pytest.raises(AssertionError):
        pkg.Engine.msm_batch(e, [bytes(96)], [[bytes(32)], []])
    with pytest.raises(AssertionError):
        pkg.Engine.msm_rows(e, bytes(96 * 2), [[bytes(32)] * 3])
