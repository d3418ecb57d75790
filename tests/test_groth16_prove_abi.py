"""The Groth16 prover's entry points (nbls_groth16_pk_create / _destroy / _params, nbls_groth16_prove, nbls_groth16_quotient, NBLS_TUNE_G16P_ROW_WAVE) without a GPU: exported
by libnbls.so, declared by the header (additions at ABI 5), bound with their argument types, and every refusal that needs no device work, against a fake context and a fake
key, with the output buffers untouched."""
import ctypes as C
import importlib
import os
import subprocess
import pytest
from test_verify_shared_abi import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'noble-bls12-381_amd')
NAMES = ['nbls_groth16_pk_create', 'nbls_groth16_pk_destroy', 'nbls_groth16_pk_params', 'nbls_groth16_pk_wiped', 'nbls_groth16_prove', 'nbls_groth16_quotient']
EINVAL = -1
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ZERO48, ZERO96 = b'\xc0' + bytes(47), b'\xc0' + bytes(95)


class FakePk(C.Structure):
    """the head of struct nbls_groth16_pk (pipelines_groth16_prove.cpp): the argument checks and the getter read these four, nothing else"""
    _fields_ = [('device', C.c_int), ('log2_n', C.c_uint), ('n_vars', C.c_size_t), ('n_public', C.c_size_t), ('rest', C.c_uint8 * 1024)]


def fake_pk(device, log2_n=3, n_vars=6, n_public=2):
    pk = FakePk()
    pk.device, pk.log2_n, pk.n_vars, pk.n_public = device, log2_n, n_vars, n_public
    return pk


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
    for nm in ('nbls_g16p_witness_launch', 'nbls_g16p_spmv_launch', 'nbls_g16p_quotient_launch', 'nbls_g16p_check_launch', 'nbls_g16p_quot_status_launch', 'nbls_g16p_scalars_launch',
               'nbls_g16p_mask_launch', 'nbls_g16p_finish_launch', 'g16p_pk_build', 'g16p_quotient_dev', 'g16p_host_matrix', 'nbls_sim_'):
        assert not any(nm in e for e in exported), nm          # the kernels' launch wrappers, the internal cores and the simulator's entries stay out
    assert lib.nbls_abi_version() == 5
    sim = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(PKG, 'libnbls_sim.so')]).decode()
    for nm in ('nbls_sim_g16p_spmv', 'nbls_sim_g16p_quotient', 'nbls_sim_g16p_scalars'):
        assert nm in sim, nm


def test_header_declares_them_at_abi_5():
    src = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert '#define NBLS_ABI_VERSION 5' in src
    assert 'typedef struct nbls_groth16_pk nbls_groth16_pk;' in src and '} nbls_groth16_pk_desc;' in src
    assert '#define NBLS_ST_G16_UNSATISFIED 24' in src and '#define NBLS_TUNE_G16P_ROW_WAVE 31' in src
    for nm in NAMES:
        assert ' ' + nm + '(' in src, nm
    flat = ' '.join(src.replace('*', ' ').split())
    assert ('scratch slot 87 (additions only, same version). Then nbls_groth16_pk_create / _destroy / _params / _wiped, nbls_groth16_prove, nbls_groth16_quotient, '
            'NBLS_ST_G16_UNSATISFIED, NBLS_TUNE_G16P_ROW_WAVE, no scratch slot (additions only, same version).') in flat
    decl = flat[flat.index('The Groth16 prover:'):flat.index('#define NBLS_ST_G16_UNSATISFIED')]
    for words in ('A = alpha_g1 + sum_i [z_i] a_query_i + [r] delta_g1', 'h_query_k = [tau^k Z(tau) / delta]G1', "bellman's ProvingKey", 'intended and untested',
                  'l_query | h_query | [slot A] | [slot B1] | delta_g1', 'A ZERO POINT (0xc0 00..) IS VALID', 'its scalar is forced to zero', 'NBLS_EDECODE, out = NULL',
                  'log2_n outside 1 .. 21', 'above 2^22', 'more than 2^24 entries in one matrix', 'a non-canonical coefficient', 'disagree on being the zero point',
                  'two contexts never prove on it at once', 'NBLS_ST_NON_CANONICAL', 'NBLS_ST_G16_UNSATISFIED', '192 ZERO BYTES', 'never disturbs its neighbours',
                  'getrandom(2)', 'NBLS_ENOSUP', 'never a fixed value', 'n = 0, n > 2^16, a key on another device', 'ARE SECRETS', "as bellman's multiexp does",
                  'the only sense in which the call is not constant time', 'any shift g with g^N != 1 gives the same h', 'UNSPECIFIED bytes', 'log2_n outside 1 .. 22',
                  'more than 2^24 elements in a row set', 'n = 0 is NBLS_OK'):
        assert words in decl, words
    internal = open(os.path.join(PKG, 'csrc', 'nbls_internal.h')).read()
    assert 'static_assert(NSB == 88' in internal          # the prover's workspace is the handle's: no scratch slot was added


def test_binding_argtypes(pkg):
    bound = pkg.load_library()
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert bound.nbls_groth16_pk_create.argtypes == [vp, C.POINTER(pkg.Groth16PkDesc), vp, C.POINTER(vp)]
    assert bound.nbls_groth16_pk_destroy.argtypes == [vp] and bound.nbls_groth16_pk_destroy.restype is None
    assert bound.nbls_groth16_pk_params.argtypes == [vp, C.POINTER(u), C.POINTER(sz), C.POINTER(sz)]
    assert bound.nbls_groth16_pk_wiped.argtypes == [vp, vp, C.POINTER(C.c_int)]
    assert bound.nbls_groth16_prove.argtypes == [vp, vp, sz, vp, vp, vp, vp]
    assert bound.nbls_groth16_quotient.argtypes == [vp, u, sz, vp, vp, vp, vp, vp]
    for m in ('groth16_pk', 'groth16_prove', 'groth16_quotient', 'groth16_pk_wiped', 'set_groth16_row_wave'):
        assert callable(getattr(pkg.Engine, m, None)), m
    assert callable(pkg.Groth16Pk.close) and all(isinstance(getattr(pkg.Groth16Pk, p), property) for p in ('log2_n', 'n_vars', 'n_public'))
    # the descriptor's layout is the header's: one unsigned, three sizes, nineteen pointers
    assert [f[0] for f in pkg.Groth16PkDesc._fields_[:4]] == ['log2_n', 'n_vars', 'n_public', 'n_constraints'] and len(pkg.Groth16PkDesc._fields_) == 23
    assert C.sizeof(pkg.Groth16PkDesc) == 4 * 8 + 19 * 8


class Desc:
    """a well-formed descriptor of a tiny instance (N = 4, 5 variables, 1 public input, 3 constraints of one entry a matrix) whose points are never decoded: every call below
    is refused before any device work"""

    def __init__(self, pkg):
        self.keep = {}
        self.d = pkg.Groth16PkDesc(log2_n=2, n_vars=5, n_public=1, n_constraints=3)
        one = (1).to_bytes(32, 'big')
        for m in 'abc':
            self.set(m + '_rows', (C.c_uint32 * 4)(0, 1, 2, 3))
            self.set(m + '_cols', (C.c_uint32 * 3)(0, 1, 4))
            self.set(m + '_vals32', C.create_string_buffer(one * 3, 96))
        for f, size in (('alpha_g1_48', 48), ('beta_g1_48', 48), ('beta_g2_96', 96), ('delta_g1_48', 48), ('delta_g2_96', 96), ('a_query48', 5 * 48), ('b_g1_query48', 5 * 48),
                        ('b_g2_query96', 5 * 96), ('l_query48', 3 * 48), ('h_query48', 3 * 48)):
            self.set(f, C.create_string_buffer(b'\x80' + bytes(size - 1), size))

    def set(self, field, buf):
        self.keep[field] = buf
        setattr(self.d, field, C.cast(buf, C.c_void_p) if buf is not None else None)


def test_key_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    h = C.c_void_p(7)
    st = C.create_string_buffer(b'\x55' * 32, 32)

    def refused(c, desc, out=True):
        h.value = 7
        r = b.nbls_groth16_pk_create(c, C.byref(desc.d) if desc is not None else None, st, C.byref(h) if out else None)
        return r == EINVAL and (not out or h.value is None)          # *out = NULL

    assert refused(None, Desc(pkg)) and refused(ctx, None) and refused(ctx, Desc(pkg), out=False)
    # a missing pointer (l_query may be missing only where there is no auxiliary variable)
    for f, _ in pkg.Groth16PkDesc._fields_[4:]:
        d = Desc(pkg)
        d.set(f, None)
        assert refused(ctx, d), f
    for field, values in (('log2_n', (0, 22, 32)), ('n_public', (0, 5, 6)), ('n_vars', (1, 0)), ('n_constraints', (5, 1 << 40))):
        for v in values:
            d = Desc(pkg)
            setattr(d.d, field, v)
            assert refused(ctx, d), (field, v)
    # n_aux + N + 2 > 2^22 and n_vars + 2 > 2^22: refused on the sizes alone, before an array of that size is read
    d = Desc(pkg)
    d.d.n_vars = (1 << 22) - 3          # n_aux = 2^22 - 5, N = 4
    assert refused(ctx, d)
    d.d.n_vars, d.d.n_public = (1 << 22) - 1, (1 << 22) - 3
    assert refused(ctx, d)
    # the matrices: offsets, columns, coefficients
    for m in 'abc':
        for rows in ((1, 1, 2, 3), (0, 2, 1, 3), (0, 1, 2, 1)):
            d = Desc(pkg)
            d.set(m + '_rows', (C.c_uint32 * 4)(*rows))
            assert refused(ctx, d), (m, rows)
        d = Desc(pkg)
        d.set(m + '_rows', (C.c_uint32 * 4)(0, 1, 2, (1 << 24) + 1))          # more than 2^24 entries
        assert refused(ctx, d), m
        d = Desc(pkg)
        d.set(m + '_cols', (C.c_uint32 * 3)(0, 5, 4))          # a column >= n_vars
        assert refused(ctx, d), m
        for v in (R, (1 << 256) - 1):
            d = Desc(pkg)
            d.set(m + '_vals32', C.create_string_buffer((1).to_bytes(32, 'big') * 2 + v.to_bytes(32, 'big'), 96))
            assert refused(ctx, d), (m, v)
    # b_g1_query[i] and b_g2_query[i] disagree on being the zero point
    for which in (0, 1):
        d = Desc(pkg)
        g1 = [b'\x80' + bytes(47)] * 5
        g2 = [b'\x80' + bytes(95)] * 5
        if which:
            g1[3] = ZERO48
        else:
            g2[4] = ZERO96
        d.set('b_g1_query48', C.create_string_buffer(b''.join(g1), 240)); d.set('b_g2_query96', C.create_string_buffer(b''.join(g2), 480))
        assert refused(ctx, d), which
    assert st.raw == b'\x55' * 32
    b.nbls_groth16_pk_destroy(None)          # a no-op
    L, nv, m = C.c_uint(7), C.c_size_t(7), C.c_size_t(7)
    pk = fake_pk(0, 3, 6, 2)
    g = b.nbls_groth16_pk_params
    assert g(None, C.byref(L), C.byref(nv), C.byref(m)) == EINVAL and g(C.byref(pk), None, C.byref(nv), C.byref(m)) == EINVAL
    assert g(C.byref(pk), C.byref(L), None, C.byref(m)) == EINVAL and g(C.byref(pk), C.byref(L), C.byref(nv), None) == EINVAL
    assert (L.value, nv.value, m.value) == (7, 7, 7)
    assert g(C.byref(pk), C.byref(L), C.byref(nv), C.byref(m)) == 0 and (L.value, nv.value, m.value) == (3, 6, 2)


def test_call_refusals_before_any_device_work(pkg):
    b = pkg.load_library()
    ctx = C.byref(FakeCtx())
    x = (1).to_bytes(32, 'big')
    out, st = C.create_string_buffer(b'\x55' * 192, 192), C.create_string_buffer(b'\x55' * 4, 4)
    pk, far = fake_pk(0), fake_pk(1)
    f = b.nbls_groth16_prove
    w, rs = x * 6, x * 2
    assert f(None, C.byref(pk), 1, w, rs, out, st) == EINVAL and f(ctx, None, 1, w, rs, out, st) == EINVAL
    assert f(ctx, C.byref(pk), 1, None, rs, out, st) == EINVAL and f(ctx, C.byref(pk), 1, w, rs, None, st) == EINVAL
    assert f(ctx, C.byref(pk), 0, w, rs, out, st) == EINVAL and f(ctx, C.byref(pk), (1 << 16) + 1, w, rs, out, st) == EINVAL
    assert f(ctx, C.byref(far), 1, w, rs, out, st) == EINVAL          # a key on another device
    wiped = C.c_int(7)
    g = b.nbls_groth16_pk_wiped
    assert g(None, C.byref(pk), C.byref(wiped)) == EINVAL and g(ctx, None, C.byref(wiped)) == EINVAL and g(ctx, C.byref(pk), None) == EINVAL
    assert g(ctx, C.byref(far), C.byref(wiped)) == EINVAL and wiped.value == 7
    q = b.nbls_groth16_quotient
    big = C.create_string_buffer(b'\x55' * 128, 128)
    for k in (0, 23, 32):
        assert q(ctx, k, 1, x * 4, x * 4, x * 4, big, st) == EINVAL, k
    assert q(None, 2, 1, x * 4, x * 4, x * 4, big, st) == EINVAL and q(None, 2, 0, None, None, None, None, None) == EINVAL
    assert q(ctx, 2, 1, None, x * 4, x * 4, big, st) == EINVAL and q(ctx, 2, 1, x * 4, None, x * 4, big, st) == EINVAL
    assert q(ctx, 2, 1, x * 4, x * 4, None, big, st) == EINVAL and q(ctx, 2, 1, x * 4, x * 4, x * 4, None, st) == EINVAL
    assert q(ctx, 12, 4097, x, x, x, big, st) == EINVAL and q(ctx, 22, 5, x, x, x, big, st) == EINVAL and q(ctx, 1, (1 << 23) + 1, x, x, x, big, st) == EINVAL
    assert q(ctx, 2, 0, None, None, None, None, None) == 0 and q(ctx, 22, 0, None, None, None, None, None) == 0
    assert out.raw == b'\x55' * 192 and st.raw == b'\x55' * 4 and big.raw == b'\x55' * 128


def test_tuning_key(pkg):
    b = pkg.load_library()
    fake = FakeCtx()
    ctx = C.byref(fake)
    x = (1).to_bytes(32, 'big')
    out = C.create_string_buffer(128)
    for v in (0, 1, 8, 1 << 30):
        assert b.nbls_set_tuning(ctx, 31, v) == 0, v
    assert b.nbls_set_tuning(ctx, 31, -1) == EINVAL and b.nbls_set_tuning(ctx, 32, 0) == EINVAL and b.nbls_set_tuning(None, 31, 1) == EINVAL
    # a tail size that leaves more than 12 global stages is refused by both calls before any device work
    assert b.nbls_set_tuning(ctx, 26, 1) == 0
    assert b.nbls_groth16_quotient(ctx, 14, 1, x, x, x, out, None) == EINVAL
    pk = fake_pk(0, 14, 6, 2)
    assert b.nbls_groth16_prove(ctx, C.byref(pk), 1, x * 6, x * 2, out, None) == EINVAL
    assert b.nbls_set_tuning(ctx, 26, 0) == 0 and b.nbls_set_tuning(ctx, 31, 0) == 0
    assert bytes(fake.raw) == bytes(1 << 16) and out.raw == bytes(128)


def test_engine_rejects_ragged_arguments(pkg):
    e = pkg.Engine.__new__(pkg.Engine)          # no device: the checks below come before any call into the library
    fake = fake_pk(0, 3, 6, 2)
    pk = pkg.Groth16Pk(pkg.load_library(), C.byref(fake))
    pk.close = lambda: None          # (not a handle the library made)
    assert (pk.log2_n, pk.n_vars, pk.n_public) == (3, 6, 2)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prove(e, pk, [[1, 2, 3]])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prove(e, pk, [])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prove(e, pk, [[1] * 6], rs=[(1, 2), (3, 4)])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prove(e, pk, [[1] * 6], rs=[(1,)])
    closed = pkg.Groth16Pk(pkg.load_library(), None)
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_prove(e, closed, [[1] * 6])
    with pytest.raises(pkg.NblsError):
        closed.n_vars
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_quotient(e, 0, bytes(64), bytes(64), bytes(64))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_quotient(e, 2, bytes(128), bytes(128), bytes(96))
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_quotient(e, 2, [[1, 2, 3]], [[1, 2, 3]], [[1, 2, 3]])
    g1, g2 = bytes(48), bytes(96)
    mats = [[[(0, 1)]], [[(0, 1)]], [[(0, 1)]]]
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_pk(e, 0, 3, 1, mats, g1, g1, g2, g1, g2, [g1] * 3, [g1] * 3, [g2] * 3, [g1], [g1])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_pk(e, 1, 3, 3, mats, g1, g1, g2, g1, g2, [g1] * 3, [g1] * 3, [g2] * 3, [g1], [g1])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_pk(e, 1, 3, 1, mats[:2], g1, g1, g2, g1, g2, [g1] * 3, [g1] * 3, [g2] * 3, [g1], [g1])
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_pk(e, 1, 3, 1, mats, g1, g1, g2, g1, g2, [g1] * 3, [g1] * 2, [g2] * 3, [g1], [g1])          # a query one point short
    with pytest.raises(pkg.NblsError):
        pkg.Engine.groth16_pk(e, 1, 3, 1, mats, g1, g1, g2, g1, g2[:95], [g1] * 3, [g1] * 3, [g2] * 3, [g1], [g1])
    pk.h = None
