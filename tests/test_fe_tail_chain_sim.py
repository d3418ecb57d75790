"""The final product of the final exponentiation in its chainable form (csrc/programs.h XP_FE_FINAL12, "fe_final12": FE_FINAL's trace served by the kernel of EXPX, so that a
pool context runs t7 = t6^x and the product as one launch) on the host simulator (CPU only): the interpreter's semantics and the translated form on the step bodies of EXPX's
kernel, on the Fp12 inputs tests/test_vm_sim.py feeds FE_FINAL -- the reference's finalExponentiate known answer and the reference-run Fp12 values -- with the same canonical
bytes expected."""
import ctypes as C
import pytest
import vmsim_py
from goldenio import hx

RAW, F12 = vmsim_py.RAW, vmsim_py.F12


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_extra_run_named.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
    lib.nbls_sim_extra_verify_named.argtypes = [C.c_char_p]
    lib.nbls_sim_extra_layout_info_named.argtypes = [C.c_char_p, C.POINTER(C.c_ulong)]
    return lib


@pytest.fixture(scope='module')
def factors(sim, golden, testdata):
    """t1 .. t7 of six final exponentiations (FE_FINAL12 runs five items a wavefront: a full one and a partly filled one), computed once with the numbered programs, and
    the bytes the reference has for them"""
    fin = [hx(testdata['finalexp_in'])] + [hx(v['a']) for v in golden['fp12'][:5]]
    want = [hx(testdata['finalexp_out'])] + [hx(v['finalexp']) for v in golden['fp12'][:5]]
    n = len(fin)
    blob = b''.join(fin)
    F, N, NI = vmsim_py.buf(F12 * n), vmsim_py.buf(RAW * n), vmsim_py.buf(RAW * n)
    T = [vmsim_py.buf(F12 * n) for _ in range(7)]
    run = lambda prog, bufs: vmsim_py.run(sim, prog, n, bufs)
    run('NORM_BYTES', {2: (vmsim_py.buf(blob), 576), 3: (F, F12), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(n), N, NI)
    run('FE_EASY', {3: (F, F12), 4: (NI, RAW), 5: (T[0], F12)})
    ex = lambda a, b: run('EXPX', {3: (a, F12), 5: (b, F12)})
    ex(T[0], T[1])
    run('FE_MID1', {3: (T[0], F12), 5: (T[1], F12), 6: (T[2], F12)})
    ex(T[2], T[3]); ex(T[3], T[4]); ex(T[4], T[6])
    run('FE_MID2', {3: (T[6], F12), 5: (T[1], F12), 6: (T[5], F12)})
    ex(T[5], T[6])
    return n, T, want


def _final(sim, n, T, name, aot):
    """the final product by a numbered program (name = 'FE_FINAL') or by the named one"""
    out = vmsim_py.buf(576 * n)
    bufs = {i: (T[i], F12) for i in range(7)}
    bufs[7] = (out, 576)
    if name == 'FE_FINAL':
        sim.nbls_sim_set_aot(aot)
        try:
            vmsim_py.run(sim, name, n, bufs)
        finally:
            sim.nbls_sim_set_aot(0)
        return out.raw
    ptrs = (C.c_void_p * 8)(); strides = (C.c_uint64 * 8)()
    for k, (b, s) in bufs.items():
        ptrs[k] = C.cast(b, C.c_void_p); strides[k] = s
    assert sim.nbls_sim_extra_run_named(name.encode(), aot, n, ptrs, strides) == 0, (name, aot)
    return out.raw


def test_program_verifies(sim):
    assert sim.nbls_sim_extra_verify_named(b'fe_final12') == 0


@pytest.mark.parametrize('aot', [0, 1], ids=['interpreted', 'translated_on_expx_bodies'])
def test_chainable_final_product_gives_the_reference_bytes(sim, factors, aot):
    n, T, want = factors
    before = [t.raw for t in T]
    got = _final(sim, n, T, 'fe_final12', aot)
    for i in range(n):
        assert got[576 * i:576 * (i + 1)] == want[i], i
    assert [t.raw for t in T] == before      # the factors are inputs only: a chain's earlier segment wrote them, nothing else may
    assert got == _final(sim, n, T, 'FE_FINAL', aot)


@pytest.mark.parametrize('n', [1, 4, 5])
def test_partly_filled_wavefronts(sim, factors, n):
    """fewer items than the fixture's: a wavefront that ends inside and on its five items, the lanes of absent items writing nothing (the bytes behind the last item stay)"""
    _, T, want = factors
    out = vmsim_py.buf(b'\xa5' * (576 * (n + 1)))
    ptrs = (C.c_void_p * 8)(); strides = (C.c_uint64 * 8)()
    for i in range(7):
        ptrs[i] = C.cast(T[i], C.c_void_p); strides[i] = F12
    ptrs[7] = C.cast(out, C.c_void_p); strides[7] = 576
    assert sim.nbls_sim_extra_run_named(b'fe_final12', 1, n, ptrs, strides) == 0
    assert out.raw[:576 * n] == b''.join(want[:n]) and out.raw[576 * n:] == b'\xa5' * 576


def test_slot_placement_row_is_current(sim):
    """aot_layout.inc has a row for the program as it compiles now, and the placement removes bank conflicts under the model (as FE_FINAL's own row does)"""
    o = (C.c_ulong * 4)()
    assert sim.nbls_sim_extra_layout_info_named(b'fe_final12', o) == 0
    has, c0, c1, floor = list(o)
    assert has == 1, 'aot_layout.inc is stale for fe_final12'
    assert floor <= c1 < c0
