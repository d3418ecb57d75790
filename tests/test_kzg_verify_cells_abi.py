"""nbls_kzg_verify_cells without a GPU: exported by libnbls.so, declared by the header (ABI 5), bound with its argument types, and every refusal that needs no device work."""
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
ZERO48 = b'\xc0' + bytes(47)


@pytest.fixture(scope='module')
def lib():
    subprocess.check_call(['make', '-s', '-C', os.path.join(PKG, 'csrc'), '../libnbls.so'])
    return C.CDLL(os.path.join(PKG, 'libnbls.so'))


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


def test_symbol_exported(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls.so')]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert 'nbls_kzg_verify_cells' in exported and hasattr(lib, 'nbls_kzg_verify_cells')
    for nm in ('nbls_kzg_cell_interp_launch', 'nbls_kzg_cell_ishifts_launch', 'nbls_kzg_cell_pre_launch', 'nbls_kzg_cell_items_launch', 'verify_cells_pipeline', 'kzg_table',
               'kzg_item_tail', 'kzg_combined_tail', 'neg_g2_wire', 'KzgFrame', 'kzg_seed', 'kzg_verdict', 'kzg_pairs_carve', 'carve'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers and the internal cores stay internal
    assert lib.nbls_abi_version() == 5


def test_header_declares_it_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'int nbls_kzg_verify_cells(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n_commitments, const uint8_t* commitments48, size_t n_cells,' in src
    flat = ' '.join(src.replace('*', ' ').split())
    assert 'then nbls_kzg_verify_cells, scratch slots 74 .. 78 (addition only, same version)' in flat
    decl = flat[flat.index('verify_cell_kzg_proof_batch: n_cells cells'):flat.index('int nbls_kzg_verify_cells(')]
    for words in ('SECRET WEIGHTS in place of its Fiat-Shamir powers', 'log2_cell <= 6 IS A DELIBERATE LIMIT', 'ZERO POINTS ARE VALID', 'never a fixed seed', 'NBLS_EDECODE',
                  'every commitment decoded once', 'a Lagrange nbls_kzg_setup is not accepted', 'NOT an interface for secrets', 'test vectors have not been run',
                  'a handle created on another device', 'n_cells > 2^20', 'n_commitments > 2^22', 'fast reject'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_kzg_verify_cells.argtypes == [vp, vp, u, sz, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), vp]
    assert callable(getattr(pkg.Engine, 'kzg_verify_cells', None))


def call(b, ctx, mo, log2_cell, n_commitments, commitments, n_cells, ci, ki, cells, proofs, tau, ok, st, seed=None):
    arr = lambda v: None if v is None else (C.c_uint32 * len(v))(*v)
    return b.nbls_kzg_verify_cells(ctx, mo, log2_cell, n_commitments, commitments, n_cells, arr(ci), arr(ki), cells, proofs, tau, seed, ok, st)


def test_every_refusal_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    mo = lambda dev, k: C.byref(FakeMonomial(dev, k, None))
    ok, st = C.c_int(77), C.create_string_buffer(b'\x55' * 4, 4)
    okp = C.byref(ok)
    x, tau = (1).to_bytes(32, 'big'), bytes(96)
    good = dict(ctx=ctx, mo=mo(0, 4), log2_cell=1, n_commitments=2, commitments=ZERO48 * 2, n_cells=2, ci=[1, 0], ki=[15, 0], cells=x * 4, proofs=ZERO48 * 2, tau=tau, ok=okp, st=st)
    bad = [dict(ctx=None), dict(mo=None), dict(commitments=None), dict(ci=None), dict(ki=None), dict(cells=None), dict(proofs=None), dict(tau=None), dict(ok=None),
           dict(n_cells=0), dict(n_commitments=0),
           dict(mo=mo(1, 4)),                              # a handle of another device
           dict(mo=mo(0, 7), log2_cell=7),                 # log2_cell > 6
           dict(mo=mo(0, 4), log2_cell=5),                 # log2_cell > log2_n
           dict(mo=mo(0, 12), log2_cell=0),                # 2^13 cells per blob
           dict(ki=[16, 0]), dict(ki=[0, 16]),             # cell_index = 2 N / c
           dict(ci=[2, 0]), dict(ci=[0, 0xffffffff]),      # commitment_index >= n_commitments
           dict(n_cells=(1 << 20) + 1),                    # the batched MSM's rows
           dict(mo=mo(0, 12), log2_cell=6, n_cells=(1 << 16) + 1),   # ... and its scalars: n_cells << log2_cell > 2^22
           dict(n_commitments=(1 << 22) + 1)]
    for change in bad:
        assert call(b, **dict(good, **change)) == EINVAL, sorted(change)
    assert call(b, **dict(good, st=None, ok=None)) == EINVAL
    assert ok.value == 77 and st.raw == b'\x55' * 4          # nothing is written on an error return


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    mo = pkg.KzgMonomialSetup(pkg.load_library(), C.byref(FakeMonomial(0, 4, None)))
    mo.close = lambda: None          # (not a handle the library made)
    x, tau = bytes(64), bytes(96)
    good = dict(monomial=mo, log2_cell=1, commitments48=[ZERO48], commitment_index=[0, 0], cell_index=[0, 1], cells=[x, x], proofs48=[ZERO48] * 2, tau_c_g2_96=tau)
    for change in (dict(cells=[]), dict(cells=[x, x[:-1]]), dict(commitment_index=[0]), dict(cell_index=[0, 1, 2]), dict(proofs48=[ZERO48]), dict(proofs48=[ZERO48, ZERO48[:-1]]),
                   dict(commitments48=[]), dict(commitments48=[bytes(47)]), dict(tau_c_g2_96=bytes(95)), dict(seed=bytes(31)), dict(log2_cell=7), dict(log2_cell=-1),
                   dict(commitment_index=[0, -1]), dict(cell_index=[0, 1 << 32]), dict(monomial=pkg.KzgMonomialSetup(pkg.load_library(), None))):
        with pytest.raises(pkg.NblsError):
            pkg.Engine.kzg_verify_cells(e, **dict(good, **change))
    mo.h = None
