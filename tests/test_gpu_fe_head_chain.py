"""The easy part of the final exponentiation at the head of the first exponentiation's launch (NBLS_TUNE_FE_HEAD_CHAIN, csrc/pipelines_pairing.cpp final_exp_pipeline) and
the issue priority of the inversion kernel's wavefronts (NBLS_TUNE_INV_PRIO): a context tuned as the pool tunes its own gives the same bytes with the head chain on as with it
off, and both are the oracle's, at item counts that end inside, on and just past a five-item wavefront and at one and two 64-lane multiples; what is launched and how it is
booked; the inversion at every priority; the pool, which sets both itself; and the binding of the chainable easy part to EXPX's kernel."""
import importlib
import pytest
import torch
from goldenio import hx

pytestmark = pytest.mark.gpu
SIZES = [1, 4, 5, 6, 9, 10, 11, 64, 65]
NMAX = max(SIZES)


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def pairs(oracle, golden):
    """the golden pairs, cycled to the largest size, on the device; the oracle's pairings of all of them (a smaller batch is a prefix)"""
    vs = golden['pairs']
    G1 = b''.join(hx(vs[i % len(vs)]['g1']) for i in range(NMAX)); G2 = b''.join(hx(vs[i % len(vs)]['g2']) for i in range(NMAX))
    ref, _ = oracle.pairing_batch(G1, G2, True, False)
    for i in range(len(vs)):      # the oracle agrees with the reference's own bytes where the fixture has them
        assert ref[576 * i:576 * (i + 1)] == hx(vs[i]['pairing']), i
    d1 = torch.frombuffer(bytearray(G1), dtype=torch.uint8).cuda(); d2 = torch.frombuffer(bytearray(G2), dtype=torch.uint8).cuda()
    return d1, d2, ref


def _pool_like(pkg, head, tail=3):
    """a single context tuned as nbls_pool_init tunes its contexts, with the head chain as given"""
    eng = pkg.Engine(0)
    eng.set_split_miller_min(0); eng.set_chain_max(0); eng.set_ls_max(0, 0); eng.set_inv_wide_max(256)
    eng.set_fe_tail_chain(tail); eng.set_fe_head_chain(head)
    return eng


@pytest.fixture(scope='module')
def engines(pkg):
    return _pool_like(pkg, 1), _pool_like(pkg, 0)


def _run(eng, n, d1, d2):
    out = torch.full((576 * n + 576,), 0xa5, dtype=torch.uint8, device='cuda')      # one item of guard bytes behind the last
    eng.pairing_batch_dev(n, d1.data_ptr(), d2.data_ptr(), out.data_ptr(), True)
    torch.cuda.synchronize()
    b = bytes(out.cpu().numpy().tobytes())
    assert b[576 * n:] == b'\xa5' * 576, 'bytes behind the last item were written'
    return b[:576 * n]


def _counted(eng, n, d1, d2):
    """one call with the launches of every numbered program counted (nbls_timing_read) and the launches that were chains (nbls_chain_launches)"""
    c0 = eng.chain_launches()
    eng.timing_enable(True)
    try:
        out = _run(eng, n, d1, d2)
        counts = {k: int(v[1]) for k, v in eng.timing_read().items()}
    finally:
        eng.timing_enable(False)
    return out, counts, eng.chain_launches() - c0


@pytest.mark.parametrize('n', SIZES)
def test_same_bytes_with_the_head_chain_on_and_off(engines, pairs, n):
    """the bytes, and what was launched: a chain is booked on its first numbered program, so the head chain books five EXPX launches and no FE_EASY; a chain that fell back to
    one launch per program (which would give the same bytes) fails here"""
    on, off = engines
    d1, d2, ref = pairs
    before = on.extra_program_launches('fe_easy12')
    a, counts, chains = _counted(on, n, d1, d2)
    assert on.extra_program_launches('fe_easy12') == before + 1
    assert chains == 3
    assert counts == {'lines_pq': 1, 'acc_fe': 1, 'fp_inv': 1, 'expx': 5}, counts      # 8 launches
    b, counts_off, chains_off = _counted(off, n, d1, d2)
    assert off.extra_program_launches('fe_easy12') == 0
    assert chains_off == 3 and counts_off == {'lines_pq': 1, 'acc_fe': 1, 'fp_inv': 1, 'fe_easy': 1, 'expx': 5}, counts_off      # 9 launches
    assert a == b
    assert a == ref[:576 * n]


def test_head_chain_without_the_middle_programs(pkg, pairs):
    """tail 1: FE_MID1 stays a launch of its own, the first chain is {fe_easy12, EXPX}"""
    d1, d2, ref = pairs
    eng = _pool_like(pkg, 1, tail=1)
    out, counts, chains = _counted(eng, 6, d1, d2)
    assert out == ref[:576 * 6]
    assert chains == 2 and eng.extra_program_launches('fe_easy12') == 1
    assert counts == {'lines_pq': 1, 'acc_fe': 1, 'fp_inv': 1, 'expx': 5, 'fe_mid1': 1, 'fe_mid2': 1}, counts


def test_settings_are_checked(engines):
    on, off = engines
    for eng in (on, off):
        assert eng.lib.nbls_set_tuning(eng.h, 29, 2) != 0 and eng.lib.nbls_set_tuning(eng.h, 29, -1) != 0
        assert eng.lib.nbls_set_tuning(eng.h, 30, 4) != 0 and eng.lib.nbls_set_tuning(eng.h, 30, -1) != 0
        assert eng.lib.nbls_set_tuning(eng.h, 24, 4) != 0
        for key in (19, 21, 23, 25, 28):
            assert eng.lib.nbls_set_tuning(eng.h, key, 0) != 0, key


@pytest.mark.parametrize('prio', [0, 1, 2, 3])
def test_inversion_at_every_priority(pkg, pairs, prio):
    """one wavefront that is partly filled, nearly full, full, and a second one; the one-element-per-lane kernel at every size (the wide form never)"""
    d1, d2, ref = pairs
    eng = _pool_like(pkg, 1)
    eng.set_inv_wide_max(0); eng.set_inv_prio(prio)
    for n in (1, 63, 64, 65):
        assert _run(eng, n, d1, d2) == ref[:576 * n], n


def test_pool_of_two_contexts(pkg, pairs):
    """four submissions of 65 pairs on two contexts, two in flight: every output buffer is the oracle's; the pool has switched the form on for its contexts"""
    d1, d2, ref = pairs
    n = NMAX
    pipe = pkg.PairingPipeline(0, 2)
    outs = [torch.zeros(576 * n, dtype=torch.uint8, device='cuda') for _ in range(4)]
    for k in range(4):
        pipe.submit(n, d1.data_ptr(), d2.data_ptr(), outs[k].data_ptr(), True)
    pipe.synchronize()
    for k in range(4):
        assert bytes(outs[k].cpu().numpy().tobytes()) == ref, 'buffer %d of the pool differs from the oracle' % k
    assert [e.extra_program_launches('fe_easy12') for e in pipe.engines] == [2, 2]
    assert [e.chain_launches() for e in pipe.engines] == [6, 6]      # two batches a context, three chains a batch: 8 launches a batch
    pipe.close()


def test_chainable_easy_part_runs_on_the_kernel_of_expx(engines):
    on, _ = engines
    assert on.extra_program_kernel('fe_easy12') == 'nbls_aot_expx'
