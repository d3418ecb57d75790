"""nbls_kzg_recover_cells and nbls_kzg_recover_cells_and_proofs without a GPU: exported by libnbls.so, declared by the header (ABI 5), bound with their argument types, and every
refusal that needs no device work."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx
from test_kzg_cells_abi import FakeMonomial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
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
    for nm in ('nbls_kzg_recover_cells', 'nbls_kzg_recover_cells_and_proofs'):
        assert nm in exported and hasattr(lib, nm)
    for nm in ('nbls_kzg_recover_launch', 'nbls_sim_kzg_recover', 'nbls_sim_', 'cells_pipeline', 'recover_args_ok', 'fr_recover'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers, the simulator and the internal cores stay internal
    assert lib.nbls_abi_version() == 5
    sim = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls_sim.so')]).decode()
    assert 'nbls_sim_kzg_recover' in sim


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert '#define NBLS_ST_BAD_CELLS 22 ' in src and '#define NBLS_ST_INCONSISTENT 23 ' in src
    assert 'int nbls_kzg_recover_cells(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, size_t n /* blobs */, const uint32_t* cell_offsets /* n + 1 */,' in src
    assert 'int nbls_kzg_recover_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint32_t* cell_offsets,' in src
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('then nbls_kzg_verify_cells, scratch slots 74 .. 78 (addition only, same version); then nbls_kzg_recover_cells, nbls_kzg_recover_cells_and_proofs, '
            'NBLS_ST_BAD_CELLS, NBLS_ST_INCONSISTENT, scratch slot 79 (additions only, same version); with the MSM calls') in flat
    decl = flat[flat.index('recover_cells_and_kzg_proofs: every cell of n blobs'):flat.index('int nbls_kzg_recover_cells(')]
    for words in ('ANY ORDER', 'ZERO POINTS ARE VALID', 'never transforms at size 2 N', 'compares the recomputed cells with EVERY given cell', 'NBLS_ST_BAD_CELLS; NBLS_ST_NON_CANONICAL',
                  'NBLS_ST_INCONSISTENT; 0', 'a neighbour is never disturbed', 'Returns NBLS_OK whatever the blobs hold', 'may be NULL only when no cell is given at all',
                  'a first offset other than 0', 'log2_n + 1 - log2_cell > 12', 'more than 2^24 elements', 'a basis created on another device', '(2 N / c) N > 2^22',
                  'NBLS_TUNE_CELLS_CHUNK', 'NOT an interface for secrets', 'test vectors have not been run'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_kzg_recover_cells.argtypes == [vp, u, u, sz, vp, vp, vp, vp, vp]
    assert bound.nbls_kzg_recover_cells_and_proofs.argtypes == [vp, vp, u, sz, vp, vp, vp, vp, vp, vp]
    assert callable(getattr(pkg.Engine, 'kzg_recover_cells', None)) and callable(getattr(pkg.Engine, 'kzg_recover_cells_and_proofs', None))
    assert bound.nbls_strerror(EINVAL)


def test_every_refusal_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    mo = lambda dev, k: C.byref(FakeMonomial(dev, k, None))
    u32 = C.c_uint32
    off, idx, x = (u32 * 2)(0, 4), (u32 * 4)(0, 1, 2, 3), bytes(256)
    out, pf, st = C.create_string_buffer(b'\x55' * 256, 256), C.create_string_buffer(b'\x55' * 384, 384), C.create_string_buffer(b'\x55' * 2, 2)
    f, g = b.nbls_kzg_recover_cells, b.nbls_kzg_recover_cells_and_proofs
    assert f(None, 2, 0, 1, off, idx, x, out, st) == EINVAL and g(None, mo(0, 2), 0, 1, off, idx, x, out, pf, st) == EINVAL          # a NULL context
    assert f(ctx, 2, 0, 0, None, None, None, None, None) == 0          # n = 0: NBLS_OK, as nbls_kzg_compute_cells
    for bad in ([2, 0, 1, None, idx, x, out, st], [2, 0, 1, off, None, x, out, st], [2, 0, 1, off, idx, None, out, st], [2, 0, 1, off, idx, x, None, st],
                [0, 0, 1, off, idx, x, out, st], [13, 6, 1, off, idx, x, out, st], [2, 3, 1, off, idx, x, out, st], [0, 0, 0, off, idx, x, out, st],
                [12, 0, 1, off, idx, x, out, st],          # 2^13 cells: more than the table of roots holds
                [2, 0, 1, (u32 * 2)(1, 4), idx, x, out, st], [2, 0, 2, (u32 * 3)(0, 4, 3), idx, x, out, st],
                [12, 6, 4097, off, idx, x, out, st]):          # more than 2^24 elements of blobs
        assert f(ctx, *bad) == EINVAL, bad[:3]
    for bad in ([None, 0, 1, off, idx, x, out, pf, st], [mo(0, 2), 0, 0, off, idx, x, out, pf, st], [mo(0, 2), 0, 1, None, idx, x, out, pf, st],
                [mo(0, 2), 0, 1, off, None, x, out, pf, st], [mo(0, 2), 0, 1, off, idx, None, out, pf, st], [mo(0, 2), 0, 1, off, idx, x, None, pf, st],
                [mo(0, 2), 0, 1, off, idx, x, out, None, st], [mo(0, 2), 3, 1, off, idx, x, out, pf, st], [mo(0, 2), 0, 1, (u32 * 2)(1, 4), idx, x, out, pf, st],
                [mo(0, 2), 0, 2, (u32 * 3)(0, 4, 3), idx, x, out, pf, st],
                [mo(1, 2), 0, 1, off, idx, x, out, pf, st],          # a basis of another device
                [mo(0, 12), 0, 1, off, idx, x, out, pf, st],          # 2^13 cells per blob
                [mo(0, 12), 2, 1, off, idx, x, out, pf, st],          # 2^11 rows of 2^12 scalars: above one pass of the batched MSM
                [mo(0, 12), 6, 4097, off, idx, x, out, pf, st]):
        assert g(ctx, *bad) == EINVAL, bad[1:3]
    assert out.raw == b'\x55' * 256 and pf.raw == b'\x55' * 384 and st.raw == b'\x55' * 2          # nothing is written on an error return


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    x = bytes(64)
    good = dict(log2_n=2, log2_cell=1, cell_indices=[[0, 1]], cells=[[x, x]])
    for change in (dict(cells=[[x]]), dict(cells=[[x, x[:-1]]]), dict(cell_indices=[[0, 1], [2, 3]]), dict(cell_indices=[[0, -1]]), dict(cell_indices=[[0, 1 << 32]]),
                   dict(log2_n=0), dict(log2_n=13), dict(log2_cell=3), dict(log2_cell=-1)):
        with pytest.raises(pkg.NblsError):
            pkg.Engine.kzg_recover_cells(e, **dict(good, **change))
    mo = pkg.KzgMonomialSetup(pkg.load_library(), C.byref(FakeMonomial(0, 2, None)))
    mo.close = lambda: None          # (not a handle the library made)
    for change in (dict(cells=[[x]]), dict(cell_indices=[], cells=[]), dict(log2_cell=3), dict(monomial=pkg.KzgMonomialSetup(pkg.load_library(), None))):
        with pytest.raises(pkg.NblsError):
            pkg.Engine.kzg_recover_cells_and_proofs(e, **dict(dict(monomial=mo, log2_cell=1, cell_indices=[[0, 1]], cells=[[x, x]]), **change))
    mo.h = None
