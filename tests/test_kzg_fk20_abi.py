"""The FK20 entry points (nbls_kzg_fk20_create / _destroy / _params, nbls_kzg_compute_cells_and_proofs_fk20, nbls_kzg_recover_cells_and_proofs_fk20) without a GPU: exported
by libnbls.so, declared by the header (additions at ABI 5), bound with their argument types, and every refusal that needs no device work, against a fake context and fake
handles, with the output buffers untouched."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx
from test_kzg_cells_abi import FakeMonomial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_kzg_fk20_create', 'nbls_kzg_fk20_destroy', 'nbls_kzg_fk20_params', 'nbls_kzg_compute_cells_and_proofs_fk20', 'nbls_kzg_recover_cells_and_proofs_fk20']
EINVAL = -1


class FakeFk20(C.Structure):
    """struct nbls_kzg_fk20 as nbls_internal.h lays it out: the argument checks read the device and the two sizes, nothing else"""
    _fields_ = [('device', C.c_int), ('log2_n', C.c_uint), ('log2_cell', C.c_uint), ('xhat', C.c_void_p), ('bsplit', C.c_void_p)]


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
    for nm in ('nbls_kzg_fk20_scalars_launch', 'nbls_kzg_fk20_row_status_launch', 'nbls_kzg_fk20_powers_launch', 'nbls_kzg_fk20_matrix_launch', 'nbls_msm_keys_map_launch',
               'msm_map_dev', 'msm_map_plans_settle', 'msm_split_scalars', 'kzg_proof_close', 'fk20_build'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers and the internal cores stay internal
    assert lib.nbls_abi_version() == 5


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_kzg_fk20 nbls_kzg_fk20;' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('nbls_msm_dev, which leaves its result on the device, is not changed. Then nbls_kzg_fk20_create / _destroy / _params, nbls_kzg_compute_cells_and_proofs_fk20, '
            'nbls_kzg_recover_cells_and_proofs_fk20, the name "endo_g1" of nbls_extra_program_kernel, scratch slots 80 .. 81 (additions only, same version).') in flat
    assert 'No FK20 (see nbls_kzg_compute_cells_and_proofs_fk20)' in flat
    decl = flat[flat.index('FK20 (Feist-Khovratovich)'):flat.index('typedef struct nbls_kzg_fk20')]
    for words in ('THE CONTRACT', 'byte for byte', 'NBLS_ST_NON_CANONICAL', 'NBLS_ST_BAD_CELLS', 'NBLS_ST_INCONSISTENT', '0xc0 00..', 'status == NULL', 'the same refusals',
                  'No butterfly network over G1', 'M groups of c terms', 'M groups of M terms', '2^22', '2^20', 'NBLS_TUNE_CELLS_CHUNK', 'a basis on another device',
                  'log2_n + 1 - log2_cell > 12', '(2 N / c) N > 2^22', 'out = NULL', "n' = 1"):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_kzg_fk20_create.argtypes == [vp, vp, u, C.POINTER(vp)]
    assert bound.nbls_kzg_fk20_destroy.argtypes == [vp] and bound.nbls_kzg_fk20_destroy.restype is None
    assert bound.nbls_kzg_fk20_params.argtypes == [vp, C.POINTER(u), C.POINTER(u)]
    assert bound.nbls_kzg_compute_cells_and_proofs_fk20.argtypes == [vp, vp, sz, vp, vp, vp, vp]
    assert bound.nbls_kzg_recover_cells_and_proofs_fk20.argtypes == [vp, vp, sz, vp, vp, vp, vp, vp, vp]
    for m in ('kzg_fk20_setup', 'kzg_compute_cells_and_proofs_fk20', 'kzg_recover_cells_and_proofs_fk20'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.KzgFk20Setup.close) and isinstance(pkg.KzgFk20Setup.log2_n, property) and isinstance(pkg.KzgFk20Setup.log2_cell, property)


def test_create_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    h = C.c_void_p(7)

    def refused(c, mo, log2_cell, out=True):
        h.value = 7
        r = b.nbls_kzg_fk20_create(c, mo, log2_cell, C.byref(h) if out else None)
        return r == EINVAL and (not out or h.value is None)          # *out = NULL on every failure

    mo = lambda dev, k: C.byref(FakeMonomial(dev, k, None))
    assert refused(None, mo(0, 2), 1) and refused(ctx, None, 1) and refused(ctx, mo(0, 2), 1, out=False)          # a missing pointer
    assert refused(ctx, mo(1, 2), 1)          # a basis on another device
    assert refused(ctx, mo(0, 2), 3)          # log2_cell > log2_n
    assert refused(ctx, mo(0, 12), 0)         # log2_n + 1 - log2_cell = 13
    assert refused(ctx, mo(0, 12), 2)         # 2^11 cells of a blob of 2^12: 2^23 scalars
    assert refused(ctx, mo(0, 11), 0)         # 2^12 cells of a blob of 2^11: 2^23 scalars
    b.nbls_kzg_fk20_destroy(None)          # a no-op
    a, c = C.c_uint(7), C.c_uint(7)
    fk = C.byref(FakeFk20(0, 5, 2, None, None))
    assert b.nbls_kzg_fk20_params(None, C.byref(a), C.byref(c)) == EINVAL and b.nbls_kzg_fk20_params(fk, None, C.byref(c)) == EINVAL
    assert b.nbls_kzg_fk20_params(fk, C.byref(a), None) == EINVAL and (a.value, c.value) == (7, 7)
    assert b.nbls_kzg_fk20_params(fk, C.byref(a), C.byref(c)) == 0 and (a.value, c.value) == (5, 2)


def test_call_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, pf, st = C.create_string_buffer(256), C.create_string_buffer(48 * 8), C.create_string_buffer(2)
    fk, far, fk12 = C.byref(FakeFk20(0, 2, 1, None, None)), C.byref(FakeFk20(1, 2, 1, None, None)), C.byref(FakeFk20(0, 12, 6, None, None))
    # the blobs form: the twin's refusals with the handle in the monomial's place
    f = b.nbls_kzg_compute_cells_and_proofs_fk20
    assert f(None, fk, 1, x * 4, out, pf, st) == EINVAL and f(ctx, None, 1, x * 4, out, pf, st) == EINVAL
    assert f(ctx, fk, 0, x * 4, out, pf, st) == EINVAL
    for k in range(3):
        args = [x * 4, out, pf]
        args[k] = None
        assert f(ctx, fk, 1, *args, st) == EINVAL, k
    assert f(ctx, far, 1, x * 4, out, pf, st) == EINVAL
    assert f(ctx, fk12, 4097, x * 4, out, pf, st) == EINVAL          # more than 2^24 elements
    # the recovery form
    g = b.nbls_kzg_recover_cells_and_proofs_fk20
    off, idx, cells = (C.c_uint32 * 2)(0, 2), (C.c_uint32 * 2)(0, 1), x * 4
    assert g(None, fk, 1, off, idx, cells, out, pf, st) == EINVAL and g(ctx, None, 1, off, idx, cells, out, pf, st) == EINVAL
    assert g(ctx, fk, 0, off, idx, cells, out, pf, st) == EINVAL
    assert g(ctx, far, 1, off, idx, cells, out, pf, st) == EINVAL
    assert g(ctx, fk, 1, None, idx, cells, out, pf, st) == EINVAL and g(ctx, fk, 1, off, None, cells, out, pf, st) == EINVAL
    assert g(ctx, fk, 1, off, idx, None, out, pf, st) == EINVAL and g(ctx, fk, 1, off, idx, cells, None, pf, st) == EINVAL
    assert g(ctx, fk, 1, off, idx, cells, out, None, st) == EINVAL
    assert g(ctx, fk, 1, (C.c_uint32 * 2)(1, 2), idx, cells, out, pf, st) == EINVAL          # a first offset other than 0
    assert g(ctx, fk, 2, (C.c_uint32 * 3)(0, 2, 1), idx, cells, out, pf, st) == EINVAL       # decreasing offsets
    assert g(ctx, fk12, 4097, (C.c_uint32 * 4098)(), None, None, out, pf, st) == EINVAL      # more than 2^24 elements of blobs
    # no new tuning key
    assert b.nbls_set_tuning(ctx, 20, 2) == 0 and b.nbls_set_tuning(ctx, 20, 0) == 0 and b.nbls_set_tuning(ctx, 21, 0) == EINVAL
    assert out.raw == bytes(256) and pf.raw == bytes(48 * 8) and st.raw == bytes(2)


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    fk = pkg.KzgFk20Setup(pkg.load_library(), C.byref(FakeFk20(0, 2, 1, None, None)))
    fk.close = lambda: None          # (not a handle the library made)
    assert (fk.log2_n, fk.log2_cell) == (2, 1)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs_fk20(e, fk, [bytes(127)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs_fk20(e, fk, [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_recover_cells_and_proofs_fk20(e, fk, [], [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_recover_cells_and_proofs_fk20(e, fk, [[0, 1]], [[bytes(64)]])
    closed = pkg.KzgFk20Setup(pkg.load_library(), None)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_compute_cells_and_proofs_fk20(e, closed, [bytes(128)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_recover_cells_and_proofs_fk20(e, closed, [[0]], [[bytes(64)]])
    mo = pkg.KzgMonomialSetup(pkg.load_library(), C.byref(FakeMonomial(0, 2, None)))
    mo.close = lambda: None
    with pytest.raises(pkg.NblsError):
        pkg.Engine.kzg_fk20_setup(e, mo, 3)
    mo.h = None
    fk.h = None
