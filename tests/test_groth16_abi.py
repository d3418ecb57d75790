"""The Groth16 entry points (nbls_groth16_vk_create / _destroy / _inputs, nbls_groth16_verify, nbls_groth16_prepare_inputs, nbls_groth16_input_sums) without a GPU: exported by
libnbls.so, declared by the header (additions at ABI 5), bound with their argument types, and every refusal that needs no device work, against a fake context and a fake key,
with the output buffers untouched."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_groth16_vk_create', 'nbls_groth16_vk_destroy', 'nbls_groth16_vk_inputs', 'nbls_groth16_verify', 'nbls_groth16_prepare_inputs', 'nbls_groth16_input_sums']
EINVAL = -1


class FakeVk(C.Structure):
    """struct nbls_groth16_vk as nbls_internal.h lays it out: the argument checks read the device and the number of inputs, nothing else"""
    _fields_ = [('device', C.c_int), ('m', C.c_size_t)] + [(nm, C.c_void_p) for nm in ('mem', 'alpha96', 'g2neg', 'tables', 'ic96', 'ic_conv', 'ic0_proj')]


def fake_vk(device, m):
    return C.byref(FakeVk(device, m, None, None, None, None, None, None, None))


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
    for nm in ('nbls_g16_input_sums_launch', 'nbls_g16_split_launch', 'nbls_g16_pre_launch', 'nbls_g16_items_launch', 'nbls_g16_rows_launch', 'nbls_g16_status_launch',
               'nbls_g16_prepare_tail_launch', 'groth16_pipeline', 'g16_vk_build', 'g16_l_points', 'nbls_sim_'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers, the internal cores and the simulator's entries stay out
    assert lib.nbls_abi_version() == 5
    sim = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls_sim.so')]).decode()
    assert 'nbls_sim_g16_input_sums' in sim


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_groth16_vk nbls_groth16_vk;' in src
    assert '#define NBLS_ST_G16_C 30' in src and '#define NBLS_TUNE_G16_CHUNK 22' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('scratch slots 80 .. 81 (additions only, same version). Then nbls_groth16_vk_create / _destroy / _inputs, nbls_groth16_verify, nbls_groth16_prepare_inputs, '
            'nbls_groth16_input_sums, NBLS_ST_G16_C, NBLS_TUNE_G16_CHUNK, scratch slots 82 .. 86 (additions only, same version).') in flat
    decl = flat[flat.index('---- Groth16 over BLS12-381'):flat.index('typedef struct nbls_groth16_vk')]
    for words in ('e(A_i, B_i) e(L_i, -gamma) e(C_i, -delta) e(alpha, -beta) = 1', 'S_0 = sum_i r_i', 'BE64(SHA-256(seed || BE64(i))[0..8]) | 2^63', 'never a fixed seed',
                  'no point is negated on the device', 'PointG1.fromHex', 'PointG2.fromSignature', "bellman's Proof::write", 'must be canonical', 'stays with the caller',
                  'alpha, beta, gamma, delta, IC_0 .. IC_m', 'NBLS_EDECODE with out = NULL', "nbls_kzg_setup_create's", 'm = 0 or m > 2^16', '10 + B', 'NBLS_ST_G16_C + C',
                  'NBLS_ST_NON_CANONICAL', 'NBLS_ST_NOT_VERIFIED', 'weight zero everywhere', 'a neighbour is never disturbed', 'fast reject', 'a zero L_i is a factor of one',
                  '2^22 scalars and 2^20 rows', 'NBLS_TUNE_G16_CHUNK', 'the bytes do not depend on the chunks', 'n = 0, n > 2^20, n m > 2^24, a key on another device',
                  'NOT written on an error return', '0xc0 00..', '48 zero bytes', 'a weight >= 2^64', 'NOT an interface for secrets'):
        assert words in decl, words


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    assert bound.nbls_groth16_vk_create.argtypes == [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    assert bound.nbls_groth16_vk_destroy.argtypes == [vp] and bound.nbls_groth16_vk_destroy.restype is None
    assert bound.nbls_groth16_vk_inputs.argtypes == [vp, C.POINTER(sz)]
    assert bound.nbls_groth16_verify.argtypes == [vp, vp, sz, vp, vp, vp, C.POINTER(i32), vp]
    assert bound.nbls_groth16_prepare_inputs.argtypes == [vp, vp, sz, vp, vp, vp]
    assert bound.nbls_groth16_input_sums.argtypes == [vp, sz, sz, vp, vp, vp, vp, vp]
    for m in ('groth16_vk', 'groth16_verify', 'groth16_prepare_inputs', 'groth16_input_sums', 'set_groth16_chunk'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.Groth16Vk.close) and isinstance(pkg.Groth16Vk.inputs, property)


def test_key_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    g1, g2 = bytes(48), bytes(96)
    h = C.c_void_p(7)
    st = C.create_string_buffer(8)

    def refused(c, m, args, out=True):
        h.value = 7
        r = b.nbls_groth16_vk_create(c, m, *args, st, C.byref(h) if out else None)
        return r == EINVAL and (not out or h.value is None)          # *out = NULL

    full = [g1, g2, g2, g2, g1 * 4]
    assert refused(None, 3, full) and refused(ctx, 3, full, out=False)
    for k in range(5):
        args = list(full)
        args[k] = None
        assert refused(ctx, 3, args), k
    assert refused(ctx, 0, full) and refused(ctx, (1 << 16) + 1, full)
    assert st.raw == bytes(8)
    b.nbls_groth16_vk_destroy(None)          # a no-op
    m = C.c_size_t(7)
    assert b.nbls_groth16_vk_inputs(None, C.byref(m)) == EINVAL and b.nbls_groth16_vk_inputs(fake_vk(0, 5), None) == EINVAL and m.value == 7
    assert b.nbls_groth16_vk_inputs(fake_vk(0, 5), C.byref(m)) == 0 and m.value == 5


def test_call_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    pf = bytes(192)
    ok, st, out = C.c_int(7), C.create_string_buffer(b'\x55' * 4, 4), C.create_string_buffer(b'\x55' * 96, 96)
    vk, far = fake_vk(0, 2), fake_vk(1, 2)
    f = b.nbls_groth16_verify
    assert f(None, vk, 1, pf, x * 2, None, C.byref(ok), st) == EINVAL and f(ctx, None, 1, pf, x * 2, None, C.byref(ok), st) == EINVAL
    assert f(ctx, vk, 1, None, x * 2, None, C.byref(ok), st) == EINVAL and f(ctx, vk, 1, pf, None, None, C.byref(ok), st) == EINVAL
    assert f(ctx, vk, 1, pf, x * 2, None, None, st) == EINVAL
    assert f(ctx, vk, 0, pf, x * 2, None, C.byref(ok), st) == EINVAL
    assert f(ctx, vk, (1 << 20) + 1, pf, x * 2, None, C.byref(ok), st) == EINVAL          # n > 2^20
    assert f(ctx, fake_vk(0, 17), 1 << 20, pf, x * 2, None, C.byref(ok), st) == EINVAL    # n * m > 2^24
    assert f(ctx, far, 1, pf, x * 2, None, C.byref(ok), st) == EINVAL                     # a key on another device
    g = b.nbls_groth16_prepare_inputs
    assert g(None, vk, 1, x * 2, out, st) == EINVAL and g(ctx, None, 1, x * 2, out, st) == EINVAL
    assert g(ctx, vk, 1, None, out, st) == EINVAL and g(ctx, vk, 1, x * 2, None, st) == EINVAL
    assert g(ctx, vk, 0, x * 2, out, st) == EINVAL and g(ctx, vk, (1 << 20) + 1, x * 2, out, st) == EINVAL
    assert g(ctx, fake_vk(0, 17), 1 << 20, x * 2, out, st) == EINVAL and g(ctx, far, 1, x * 2, out, st) == EINVAL
    s = b.nbls_groth16_input_sums
    assert s(None, 1, 2, x * 2, x, None, out, st) == EINVAL
    assert s(ctx, 0, 2, x * 2, x, None, out, st) == EINVAL and s(ctx, 1, 0, x * 2, x, None, out, st) == EINVAL
    assert s(ctx, 1, 2, None, x, None, out, st) == EINVAL and s(ctx, 1, 2, x * 2, None, None, out, st) == EINVAL and s(ctx, 1, 2, x * 2, x, None, None, st) == EINVAL
    assert s(ctx, 1 << 13, (1 << 11) + 1, x * 2, x, None, out, st) == EINVAL               # n * m > 2^24, refused before a weight is read
    assert s(ctx, 1 << 40, 1 << 40, x * 2, x, None, out, st) == EINVAL                     # (a product that would wrap)
    assert s(ctx, 1, 2, x * 2, (1 << 64).to_bytes(32, 'big'), None, out, st) == EINVAL     # a weight >= 2^64
    assert s(ctx, 2, 1, x * 2, x + (1 << 255).to_bytes(32, 'big'), None, out, st) == EINVAL
    assert ok.value == 7 and st.raw == b'\x55' * 4 and out.raw == b'\x55' * 96          # nothing written on an error return


def test_tuning_key(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    assert b.nbls_set_tuning(ctx, 22, 2) == 0 and b.nbls_set_tuning(ctx, 22, 0) == 0 and b.nbls_set_tuning(ctx, 22, -1) == EINVAL
    assert b.nbls_set_tuning(ctx, 19, 0) == EINVAL and b.nbls_set_tuning(ctx, 21, 0) == EINVAL and b.nbls_set_tuning(ctx, 23, 0) == EINVAL


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    vk = pkg.Groth16Vk(pkg.load_library(), fake_vk(0, 2))
    vk.close = lambda: None          # (not a handle the library made)
    assert vk.inputs == 2
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_verify(e, vk, [bytes(192)], [[1, 2, 3]])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_verify(e, vk, [bytes(191)], [[1, 2]])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_verify(e, vk, [bytes(192)], [[1, 2]], seed=bytes(31))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_verify(e, vk, [], [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prepare_inputs(e, vk, [[1]])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_input_sums(e, [[1, 2], [3]], [1, 1])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_input_sums(e, [[1, 2]], [1, 1])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_vk(e, bytes(48), bytes(96), bytes(96), bytes(95), [bytes(48)] * 3)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_vk(e, bytes(48), bytes(96), bytes(96), bytes(96), [bytes(48)])          # m = 0
    closed = pkg.Groth16Vk(pkg.load_library(), None)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_verify(e, closed, [bytes(192)], [[1, 2]])
    vk.h = None
