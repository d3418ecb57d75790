"""The programs of a pairing that ends in the final exponentiation, on the host simulator (CPU only), in the interpreter's and in the translated (ahead-of-time) form:
`lines_fe` (csrc/programs.h XP_LINES_FE: the reference's lines times Fp2 factors, R any representative) in front of ACC_FE and the final-exponentiation programs, and
FE_FINAL as one chain of nine factors.  What a caller sees -- pairing(P, Q) as wire bytes -- must be the reference's, bit for bit; the line TABLE is free to differ, and does."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import goldenio
import vmsim_py
from goldenio import hx

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
LINE_BYTES = 68 * 6 * vmsim_py.RAW
F12, RAW = vmsim_py.F12, vmsim_py.RAW


@pytest.fixture(scope='module', params=[0, 1], ids=['interpreter', 'translated'])
def sim(request):
    lib = vmsim_py.load()
    lib.nbls_sim_set_aot(request.param)
    lib.aot = request.param
    yield lib
    lib.nbls_sim_set_aot(0)


def _run_extra(lib, name, n, bufs, aot):
    ptrs = (C.c_void_p * 8)(); strides = (C.c_uint64 * 8)()
    for k, (b, s) in bufs.items():
        ptrs[k] = C.cast(b, C.c_void_p); strides[k] = s
    assert lib.nbls_sim_extra_run_named(name.encode(), aot, C.c_uint(n), ptrs, strides) == 0, name


def _lines(lib, g1, g2, n, aot, program=None):
    """the line tables of n pairs by the program pairing_core picks for a call with final exponentiation (csrc/pipelines_pairing.cpp), or by the one named"""
    L = C.create_string_buffer(LINE_BYTES * n)
    bufs = {0: (vmsim_py.buf(g1), 96), 1: (vmsim_py.buf(g2), 192), 3: (L, LINE_BYTES)}
    if program is None:
        program = 'lines_fe' if lib.nbls_sim_lines_fe_enabled() else 'LINES_PQ'
    if program == 'lines_fe':
        _run_extra(lib, 'lines_fe', n, bufs, aot)
    else:
        vmsim_py.run(lib, program, n, bufs)
    return L


def _pairings(lib, g1, g2, aot, program=None):
    n = len(g1) // 96
    L = _lines(lib, g1, g2, n, aot, program)
    F, N, out = vmsim_py.buf(F12 * n), vmsim_py.buf(RAW * n), vmsim_py.buf(576 * n)
    vmsim_py.run(lib, 'ACC_FE', n, {3: (L, LINE_BYTES), 5: (F, F12), 4: (N, RAW)})
    vmsim_py.final_exp(lib, n, F, N, out)
    return out.raw, L.raw


def test_new_programs_pass_the_static_verifier(sim):
    """verify_program: every LDS offset, descriptor read, buffer offset and the column budget of every step, before the first run"""
    assert sim.nbls_sim_extra_verify_named(b'lines_fe') == 0
    msg = C.create_string_buffer(512)
    assert sim.nbls_sim_verify(vmsim_py.P['FE_FINAL'], msg, 512) == 0, msg.value
    assert sim.nbls_sim_has_aot(vmsim_py.P['FE_FINAL']) == 1
    assert sim.nbls_sim_program_lanes(vmsim_py.P['FE_FINAL']) == 12          # the chain: five items per wavefront
    assert sim.nbls_sim_lines_fe_enabled() == 1


def test_golden_pairs_through_lines_fe(sim, golden):
    """every reference-generated pair (LINES runs 6 items per wavefront, ACC_FE and FE_FINAL 5: partly filled last wavefronts in all of them)"""
    pairs = golden['pairs']
    n = len(pairs)
    assert n >= 11
    g1 = b''.join(hx(v['g1']) for v in pairs); g2 = b''.join(hx(v['g2']) for v in pairs)
    out, table = _pairings(sim, g1, g2, sim.aot)
    for i, v in enumerate(pairs):
        assert out[576 * i:576 * (i + 1)] == hx(v['pairing']), i
    # the table is NOT the reference's (that is the point), yet LINES_PQ's gives the same pairings
    out_pq, table_pq = _pairings(sim, g1[:96 * 2], g2[:192 * 2], sim.aot, 'LINES_PQ')
    assert out_pq == out[:576 * 2] and table_pq != table[:LINE_BYTES * 2]


def test_seeded_pairs_against_the_oracle(sim, oracle):
    """12 pairs [a]G1, [b]G2: either point the generator, the scalars 1, 2 and r - 1 on either side, and seeded random scalars"""
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    rnd = lambda tag: int.from_bytes(hashlib.sha256(b'lines-fe-' + tag).digest(), 'big') % (R_ORDER - 1) + 1
    ab = [(1, 1), (1, rnd(b'q0')), (rnd(b'p0'), 1), (2, 2), (2, rnd(b'q1')), (rnd(b'p1'), 2), (R_ORDER - 1, R_ORDER - 1), (R_ORDER - 1, rnd(b'q2')), (rnd(b'p2'), R_ORDER - 1),
          (rnd(b'p3'), rnd(b'q3')), (rnd(b'p4'), rnd(b'q4')), (rnd(b'p5'), rnd(b'q5'))]
    assert len(ab) == 12
    g1 = b''.join(oracle.g1_mul(G1, a)[1] for a, _ in ab); g2 = b''.join(oracle.g2_mul(G2, b)[1] for _, b in ab)
    assert g1[:96] == G1 and g2[:192] == G2
    ref, _ = oracle.pairing_batch(g1, g2, True, False, threads=4)
    out, _ = _pairings(sim, g1, g2, sim.aot)
    for i in range(len(ab)):
        assert out[576 * i:576 * (i + 1)] == ref[576 * i:576 * (i + 1)], ab[i]


def _fe_final_cases(lib, golden, testdata):
    """inputs t1 .. t7 of FE_FINAL, one buffer per factor: (a) the factors the pipeline really produces from the reference's finalExponentiate known answer and a reference-run
    Fp12 value, (b) ONE seven times, (c) the extreme elements of test_translated_expx_on_extreme_elements (random, all p - 1, ONE) rotated through the seven places -- the
    program is a polynomial identity in its inputs (the Frobenius map is a ring homomorphism), so both forms agree on ANY seven elements, unitary or not"""
    import random
    fin = hx(testdata['finalexp_in']) + hx(golden['fp12'][0]['a'])
    n0 = 2
    F, N, NI = vmsim_py.buf(F12 * n0), vmsim_py.buf(RAW * n0), vmsim_py.buf(RAW * n0)
    T = [vmsim_py.buf(F12 * n0) for _ in range(7)]
    run = lambda prog, bufs: vmsim_py.run(lib, prog, n0, bufs)
    run('NORM_BYTES', {2: (vmsim_py.buf(fin), 576), 3: (F, F12), 4: (N, RAW)})
    lib.nbls_sim_fp_inv(C.c_uint(n0), N, NI)
    run('FE_EASY', {3: (F, F12), 4: (NI, RAW), 5: (T[0], F12)})          # the launch sequence of final_exp_pipeline() (csrc/pipelines_pairing.cpp), stopped in front of FE_FINAL
    ex = lambda a, b: run('EXPX', {3: (a, F12), 5: (b, F12)})
    ex(T[0], T[1]); run('FE_MID1', {3: (T[0], F12), 5: (T[1], F12), 6: (T[2], F12)})
    ex(T[2], T[3]); ex(T[3], T[4]); ex(T[4], T[6])
    run('FE_MID2', {3: (T[6], F12), 5: (T[1], F12), 6: (T[5], F12)}); ex(T[5], T[6])
    p = vmsim_py.P_MOD
    rnd = random.Random(7)
    vals = [[rnd.randrange(p) for _ in range(12)] for _ in range(4)] + [[p - 1] * 12, [1] + [0] * 11]
    elem = lambda v: b''.join(vmsim_py.raw_elem(x) for x in v)
    one = elem([1] + [0] * 11)
    cols = []
    for i in range(7):
        cols.append(T[i].raw + one + b''.join(elem(vals[(k + i) % 6]) for k in range(6)))
    return cols, n0 + 1 + 6


def _fe_final_outputs(lib, golden, testdata):
    cols, n = _fe_final_cases(lib, golden, testdata)
    out = vmsim_py.buf(576 * n)
    bufs = {i: (vmsim_py.buf(cols[i]), F12) for i in range(7)}
    bufs[7] = (out, 576)
    vmsim_py.run(lib, 'FE_FINAL', n, bufs)
    return out.raw


def test_fe_final_chain_equals_the_product_tree(sim, golden, testdata):
    """FE_FINAL as a chain of nine factors against the program it replaces (NBLS_FE_FINAL_CHAIN=0, a fresh process: the switch is read when the program is compiled; the
    tree runs on the interpreter there -- the kernel's signature table is generated for the chain, as it is for the default side of every formula switch)"""
    new = _fe_final_outputs(sim, golden, testdata)
    assert new[:576] == hx(testdata['finalexp_out']) and new[576:2 * 576] == hx(golden['fp12'][0]['finalexp'])
    assert new[2 * 576:3 * 576] == (1).to_bytes(48, 'big') + bytes(528)
    env = dict(os.environ, NBLS_FE_FINAL_CHAIN='0', NBLS_SIM_NO_REBUILD='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'fe_final', '0'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('FE_FINAL ')][-1].split()
    assert line[1] == 'W=32', line[1]           # the child really ran the tree on 32 lanes
    assert bytes.fromhex(line[2]) == new


def test_switch_off_reproduces_the_parent_line_tables(sim, golden):
    """NBLS_LINES_FE=0: a call with final exponentiation takes LINES_PQ again -- the reference's own line tables, the bytes before this program existed -- and the same pairings"""
    env = dict(os.environ, NBLS_LINES_FE='0', NBLS_SIM_NO_REBUILD='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'lines', str(sim.aot)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('LINES ')][-1].split()
    n = 7
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:n]); g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:n])
    out_pq, table_pq = _pairings(sim, g1, g2, sim.aot, 'LINES_PQ')
    assert line[1] == 'enabled=0'
    assert line[2] == hashlib.sha256(table_pq).hexdigest() and bytes.fromhex(line[3]) == out_pq
    assert out_pq == b''.join(hx(v['pairing']) for v in golden['pairs'][:n])
    assert hashlib.sha256(_lines(sim, g1, g2, n, sim.aot).raw).hexdigest() != line[2]      # this process runs lines_fe


def test_slot_placement_rows_of_the_new_programs(sim):
    """csrc/aot_layout.inc has current rows for lines_fe and the chained FE_FINAL, and they remove conflict cycles under the LDS bank model (tests/test_aot_sim.py checks the others)"""
    o = (C.c_ulong * 4)()
    assert sim.nbls_sim_extra_layout_info_named(b'lines_fe', o) == 0
    assert o[0] == 1 and o[2] < o[1], list(o)
    assert sim.nbls_sim_layout_info(vmsim_py.P['FE_FINAL'], o) == 0
    assert o[0] == 1 and o[2] < o[1], list(o)


if __name__ == '__main__':      # the child of the two switch tests: prints what the parent compares
    what, aot = sys.argv[1], int(sys.argv[2])
    lib = vmsim_py.load()
    lib.nbls_sim_set_aot(aot)
    gold = goldenio.load('ref_vectors.json.gz')
    if what == 'fe_final':
        out = _fe_final_outputs(lib, gold, goldenio.load('ref_testdata.json.gz'))
        print('FE_FINAL W=%d %s' % (lib.nbls_sim_program_lanes(vmsim_py.P['FE_FINAL']), out.hex()))
    else:
        n = 7
        g1 = b''.join(hx(v['g1']) for v in gold['pairs'][:n]); g2 = b''.join(hx(v['g2']) for v in gold['pairs'][:n])
        out, table = _pairings(lib, g1, g2, aot)
        print('LINES enabled=%d %s %s' % (lib.nbls_sim_lines_fe_enabled(), hashlib.sha256(table).hexdigest(), out.hex()))
