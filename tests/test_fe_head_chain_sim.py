"""The easy part of the final exponentiation in its chainable form (csrc/programs.h XP_FE_EASY12, "fe_easy12": FE_EASY's trace at twelve lanes per item, served by the kernel
of EXPX, so that a pool context runs the easy part and t2 = t1^x as one launch) on the host simulator (CPU only): the interpreter's semantics and the translated form on the
step bodies of EXPX's kernel, with the slot placement of aot_layout.inc and with the slots as compiled, on the reference's Miller values of the golden pairs and on f = ONE.
t1 is the field element FE_EASY computes (the two programs are scheduled differently, so a raw limb vector may differ by a multiple of p), and carried through the numbered
programs it gives the reference's pairing bytes."""
import ctypes as C
import pytest
import vmsim_py
from goldenio import hx

RAW, F12, P_MOD = vmsim_py.RAW, vmsim_py.F12, vmsim_py.P_MOD
ONE = (1).to_bytes(48, 'big') + bytes(576 - 48)
FORMS = {'interpreted': 0, 'translated_placed': 1, 'translated_as_compiled': 2}


@pytest.fixture(scope='module')
def sim():
    lib = vmsim_py.load()
    lib.nbls_sim_extra_run_named.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
    lib.nbls_sim_extra_verify_named.argtypes = [C.c_char_p]
    lib.nbls_sim_extra_stats_named.argtypes = [C.c_char_p]
    lib.nbls_sim_extra_layout_info_named.argtypes = [C.c_char_p, C.POINTER(C.c_ulong)]
    return lib


def _field(raw):
    """raw elements (14 limbs of 28 bits in 16 words each, any representative) -> residues mod p"""
    out = []
    for k in range(len(raw) // RAW):
        w = raw[RAW * k:RAW * (k + 1)]
        out.append(sum(int.from_bytes(w[4 * i:4 * i + 4], 'little') << (28 * i) for i in range(14)) % P_MOD)
    return out


@pytest.fixture(scope='module')
def easy(sim, golden):
    """six final exponentiations up to the inversion (fe_easy12 runs five items a wavefront: a full one and a partly filled one): raw f, the inverse norms, FE_EASY's t1, and
    the bytes the reference has for the pairings"""
    vs = golden['pairs'][:5]
    fin = [hx(v['miller']) for v in vs] + [ONE]
    want = [hx(v['pairing']) for v in vs] + [ONE]
    n = len(fin)
    F, N, NI, T1 = vmsim_py.buf(F12 * n), vmsim_py.buf(RAW * n), vmsim_py.buf(RAW * n), vmsim_py.buf(F12 * n)
    vmsim_py.run(sim, 'NORM_BYTES', n, {2: (vmsim_py.buf(b''.join(fin)), 576), 3: (F, F12), 4: (N, RAW)})
    sim.nbls_sim_fp_inv(C.c_uint(n), N, NI)
    vmsim_py.run(sim, 'FE_EASY', n, {3: (F, F12), 4: (NI, RAW), 5: (T1, F12)})
    return n, F, NI, T1, want


def _easy12(sim, n, F, NI, aot, out=None):
    out = out or vmsim_py.buf(F12 * n)
    ptrs = (C.c_void_p * 8)(); strides = (C.c_uint64 * 8)()
    for k, (b, s) in {3: (F, F12), 4: (NI, RAW), 5: (out, F12)}.items():
        ptrs[k] = C.cast(b, C.c_void_p); strides[k] = s
    assert sim.nbls_sim_extra_run_named(b'fe_easy12', aot, n, ptrs, strides) == 0, aot
    return out


def _rest(sim, n, t1):
    """t1 -> wire bytes by the numbered programs (the launches of final_exp_pipeline behind the easy part)"""
    T = [t1] + [vmsim_py.buf(F12 * n) for _ in range(6)]
    run = lambda prog, bufs: vmsim_py.run(sim, prog, n, bufs)
    ex = lambda a, b: run('EXPX', {3: (a, F12), 5: (b, F12)})
    ex(T[0], T[1])
    run('FE_MID1', {3: (T[0], F12), 5: (T[1], F12), 6: (T[2], F12)})
    ex(T[2], T[3]); ex(T[3], T[4]); ex(T[4], T[6])
    run('FE_MID2', {3: (T[6], F12), 5: (T[1], F12), 6: (T[5], F12)})
    ex(T[5], T[6])
    out = vmsim_py.buf(576 * n)
    bufs = {i: (T[i], F12) for i in range(7)}
    bufs[7] = (out, 576)
    run('FE_FINAL', bufs)
    return out.raw


def test_program_verifies(sim):
    assert sim.nbls_sim_extra_verify_named(b'fe_easy12') == 0


@pytest.mark.parametrize('form', sorted(FORMS))
def test_chainable_easy_part_gives_fe_easys_t1_and_the_reference_bytes(sim, easy, form):
    n, F, NI, T1, want = easy
    before = (F.raw, NI.raw)
    got = _easy12(sim, n, F, NI, FORMS[form])
    assert (F.raw, NI.raw) == before      # inputs only
    assert _field(got.raw) == _field(T1.raw)
    out = _rest(sim, n, got)
    for i in range(n):
        assert out[576 * i:576 * (i + 1)] == want[i], i


@pytest.mark.parametrize('n', [1, 4, 5])
def test_partly_filled_wavefronts(sim, easy, n):
    """fewer items than the fixture's: a wavefront that ends inside and on its five items, the lanes of absent items writing nothing (the bytes behind the last item stay)"""
    _, F, NI, T1, _ = easy
    out = vmsim_py.buf(b'\xa5' * (F12 * (n + 1)))
    _easy12(sim, n, F, NI, 1, out)
    assert _field(out.raw[:F12 * n]) == _field(T1.raw[:F12 * n]) and out.raw[F12 * n:] == b'\xa5' * F12


def test_slot_placement_row_is_current_and_the_image_is_no_larger_than_the_final_products(sim, capfd):
    """aot_layout.inc has a row for the program as it compiles now and the placement removes bank conflicts under the model; a chain launch takes the largest LDS image of its
    segments, and at most fe_final12's 36 slots keep twelve workgroups a CU for every launch of EXPX's kernel"""
    o = (C.c_ulong * 4)()
    assert sim.nbls_sim_extra_layout_info_named(b'fe_easy12', o) == 0
    has, c0, c1, floor = list(o)
    assert has == 1, 'aot_layout.inc is stale for fe_easy12'
    assert floor <= c1 < c0
    slots = {}
    for name in (b'fe_easy12', b'fe_final12'):
        assert sim.nbls_sim_extra_stats_named(name) == 0
    C.CDLL(None).fflush(None)
    for line in capfd.readouterr().out.splitlines():
        w = line.split()
        if w and w[0] in ('fe_easy12', 'fe_final12'):
            slots[w[0]] = int(line.split('slots=')[1].split()[0])
    assert slots['fe_final12'] == 36 and slots['fe_easy12'] <= 36, slots
