"""On the device: the two-program Miller loop of a call that ends in the final exponentiation takes its line tables from `lines_fe` (csrc/programs.h XP_LINES_FE) and finishes in
FE_FINAL as a chain of nine factors at five items per wavefront.  nbls_pairing_batch_dev with set_split_miller_min(0) at batch sizes that leave the last wavefront of the
10 x 6 (lines), 12 x 5 (ACC_FE, EXPX, FE_FINAL) shapes partly filled, the first size that takes the two-program form by default, a two-context pool, and pairing(P, Q, false),
whose bytes stay the reference's own representatives.  One oracle run, shared."""
import hashlib
import importlib
import os
import subprocess
import sys
import pytest
import torch
from goldenio import hx

pytestmark = pytest.mark.gpu
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_MAX = 4097


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def pairs(oracle):
    """4097 distinct pairs from 64 x 64 points (the generators and the scalars 1, 2, r - 1 among them, in the first places) and the oracle's pairings of all of them"""
    G1, G2 = oracle.g1_generator(), oracle.g2_generator()
    k = lambda tag, i: int.from_bytes(hashlib.sha256(b'gpu-lines-fe-%s%d' % (tag, i)).digest(), 'big') % (R_ORDER - 1) + 1
    a = [1, 2, R_ORDER - 1] + [k(b'a', i) for i in range(61)]
    b = [1, 2, R_ORDER - 1] + [k(b'b', i) for i in range(61)]
    P = [oracle.g1_mul(G1, x)[1] for x in a]; Q = [oracle.g2_mul(G2, x)[1] for x in b]
    idx = [(i % 64, (i + i // 64) % 64) for i in range(N_MAX - 1)] + [(63, 62)]         # (i, i + j): 4096 distinct combinations, one more that differs from its neighbours
    g1 = b''.join(P[i] for i, _ in idx); g2 = b''.join(Q[j] for _, j in idx)
    ref, _ = oracle.pairing_batch(g1, g2, True, False, threads=min(16, os.cpu_count() or 8))
    d1 = torch.frombuffer(bytearray(g1), dtype=torch.uint8).cuda(); d2 = torch.frombuffer(bytearray(g2), dtype=torch.uint8).cuda()
    return d1, d2, ref


@pytest.mark.parametrize('n', [1, 5, 6, 7, 31, 61, N_MAX])
def test_batch_sizes_against_the_oracle(pkg, pairs, n):
    d1, d2, ref = pairs
    eng = pkg.Engine(0)
    if n != N_MAX:
        eng.set_split_miller_min(0)        # (4097 pairs take the two-program form by default)
    assert eng.extra_program_kernel('lines_fe') == 'nbls_aot_lines_fe' and eng.program_kernel('fe_final') == 'nbls_aot_fe_final'
    out = torch.zeros(576 * n, dtype=torch.uint8, device='cuda')
    eng.timing_enable(True)
    eng.pairing_batch_dev(n, d1.data_ptr(), d2.data_ptr(), out.data_ptr(), True, None)
    torch.cuda.synchronize()
    tm = eng.timing_read(); eng.timing_enable(False)
    assert tm['lines_pq'][1] == 1 and tm['acc_fe'][1] == 1 and tm.get('miller_fe', (0, 0))[1] == 0, tm       # the two-program form ran (lines_fe is booked in the slot of its stage)
    assert eng.extra_program_launches('lines_fe') == 1 and eng.extra_program_launches('no_such_program') == -1      # and its lines came from lines_fe, not from lines_pq
    got = bytes(out.cpu().numpy().tobytes())
    for i in range(n):
        assert got[576 * i:576 * (i + 1)] == ref[576 * i:576 * (i + 1)], (n, i)
    eng.close()


def test_two_context_pool(pkg, pairs):
    d1, d2, ref = pairs
    n, D = 64, 2
    pipe = pkg.PairingPipeline(0, D)
    outs = [torch.zeros(576 * n, dtype=torch.uint8, device='cuda') for _ in range(D)]
    for _ in range(3):
        for _ in range(D):
            pipe.submit(n, d1.data_ptr(), d2.data_ptr(), outs[pipe.slot].data_ptr(), True)
    pipe.synchronize()
    torch.cuda.synchronize()
    assert [e.extra_program_launches('lines_fe') for e in pipe.engines] == [3] * D
    for k in range(D):
        assert bytes(outs[k].cpu().numpy().tobytes()) == ref[:576 * n], 'buffer %d of the pool differs from the oracle' % k
    pipe.close()


def test_miller_only_is_still_the_reference_representative(pkg, golden):
    """with_final_exp = 0 keeps LINES_PQ: the conjugated Miller value of the reference, bit for bit"""
    n = 7
    g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:n]); g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:n])
    d1 = torch.frombuffer(bytearray(g1), dtype=torch.uint8).cuda(); d2 = torch.frombuffer(bytearray(g2), dtype=torch.uint8).cuda()
    out = torch.zeros(576 * n, dtype=torch.uint8, device='cuda')
    eng = pkg.Engine(0)
    eng.set_split_miller_min(0)
    eng.pairing_batch_dev(n, d1.data_ptr(), d2.data_ptr(), out.data_ptr(), False, None)
    torch.cuda.synchronize()
    assert eng.extra_program_launches('lines_fe') == 0
    got = bytes(out.cpu().numpy().tobytes())
    for i in range(n):
        assert got[576 * i:576 * (i + 1)] == hx(golden['pairs'][i]['miller']), i
    eng.close()


CHILD = r'''
import importlib, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import torch
import goldenio
from goldenio import hx
pkg = importlib.import_module('noble-bls12-381_amd')
golden = goldenio.load('ref_vectors.json.gz')
n = 7
g1 = b''.join(hx(v['g1']) for v in golden['pairs'][:n]); g2 = b''.join(hx(v['g2']) for v in golden['pairs'][:n])
eng = pkg.Engine(0)
eng.set_split_miller_min(0)
out, _ = eng.pairing_batch(g1, g2, True, False)
assert out == b''.join(hx(v['pairing']) for v in golden['pairs'][:n])
print('CHILD_OK lines_fe_launches=%%d fe_final=%%s %%s' %% (eng.extra_program_launches('lines_fe'), eng.program_kernel('fe_final'), eng.config_describe()))
'''


@pytest.mark.parametrize('env,launches,fe_final', [({'NBLS_LINES_FE': '0'}, 0, 'nbls_aot_fe_final'), ({'NBLS_FE_FINAL_CHAIN': '0'}, 1, 'nbls_vm_kernel')])
def test_switches_on_the_device(env, launches, fe_final):
    """NBLS_LINES_FE=0: pairing_core launches lines_pq and never lines_fe; NBLS_FE_FINAL_CHAIN=0: FE_FINAL is the product tree, on the interpreter (the kernel's signature table
    is generated for the chain).  Either way the reference's pairings, bit for bit.  A fresh process each: the switches are read once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, '-c', CHILD % {'root': root}], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'CHILD_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith('CHILD_OK')][-1]
    assert 'lines_fe_launches=%d ' % launches in line and 'fe_final=%s ' % fe_final in line, line
    for k, v in env.items():
        assert '%s=%s(env)' % (k, v) in line, line


def test_no_ahead_of_time_kernel_uses_scratch_memory(pkg):
    """every kernel of aot_kernel.hip as loaded on the device: no private segment (the lane number used to be spilled across the step loop in the kernels with an eight-round body)"""
    eng = pkg.Engine(0)
    eng.program_kernel('expx')          # the module is loaded
    sizes = {}
    k = 0
    while True:
        b = eng.lib.nbls_aot_kernel_private_bytes(k)
        if b == -1:
            break
        sizes[k] = b; k += 1
    assert k >= 35 and all(v == 0 for v in sizes.values()), sizes
    eng.close()
