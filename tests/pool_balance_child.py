"""Child process of tests/test_gpu_pool_balance.py: a submit of a balanced pool may wait, and a wait that never ends must fail the test instead of hanging the suite, so
every case runs here under the parent's time limit; NBLS_POOL_MAX_OUTSTANDING is read once per process as well.  argv: one or more of `balance`, `plain`.  Per mode: a pool
of depth 4, 40 submits of n = 64 pairings, every submit into a buffer of its own.  Prints one JSON line: per mode, the slots announced (None where the submit was made with
no nbls_pool_next_slot before it), the slots the submits reported, the largest nbls_pool_outstanding seen after any submit (and after the synchronise), and how many of the
40 buffers differ from the oracle."""
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DEPTH, N, SUBMITS = 4, 64, 40


def outstanding(pipe):
    out = []
    for i in range(pipe.depth):
        v = C.c_int(-1)
        assert pipe.lib.nbls_pool_outstanding(pipe.h, i, C.byref(v)) == 0
        out.append(v.value)
    return out


def scenario(pkg, balance, d1, d2, ref):
    pipe = pkg.PairingPipeline(0, DEPTH, balance=balance)
    outs = [torch.zeros(576 * N, dtype=torch.uint8, device='cuda') for _ in range(SUBMITS)]
    announced, reported, seen = [], [], []
    torch.cuda.synchronize()
    for i in range(SUBMITS):
        if i % 5 == 4:      # a submit with no next_slot before it chooses for itself
            announced.append(None)
        else:
            a = pipe.slot
            assert pipe.slot == a, 'two nbls_pool_next_slot calls in a row gave different slots'
            announced.append(a)
        s = C.c_int(-1)
        r = pipe.lib.nbls_pool_pairing_batch_dev(pipe.h, N, d1.data_ptr(), d2.data_ptr(), 1, outs[i].data_ptr(), C.byref(s))
        assert r == 0, r
        reported.append(s.value)
        seen.append(outstanding(pipe))
    pipe.synchronize()
    after_sync = outstanding(pipe)
    v = C.c_int()
    bad_index = [pipe.lib.nbls_pool_outstanding(pipe.h, -1, C.byref(v)), pipe.lib.nbls_pool_outstanding(pipe.h, DEPTH, C.byref(v)), pipe.lib.nbls_pool_outstanding(pipe.h, 0, None)]
    differ = sum(int(bytes(o.cpu().numpy().tobytes()) != ref) for o in outs)
    pipe.close()
    return {'announced': announced, 'reported': reported, 'max_outstanding': max(max(s) for s in seen), 'min_outstanding': min(min(s) for s in seen),
            'outstanding_after_sync': after_sync, 'bad_index': bad_index, 'differ_from_oracle': differ, 'buffers': len(outs)}


def main():
    pkg = importlib.import_module('noble-bls12-381_amd')
    import bench
    import oracle_py
    oracle = oracle_py.load()
    eng = pkg.Engine(0)
    G1, G2 = bench.synth_stream(eng, oracle, N, seed=0x62616c61)
    eng.close()
    ref, _ = oracle.pairing_batch(G1, G2, True, False, threads=min(16, os.cpu_count() or 8))
    d1 = torch.frombuffer(bytearray(G1), dtype=torch.uint8).cuda(); d2 = torch.frombuffer(bytearray(G2), dtype=torch.uint8).cuda()
    res = {'max_outstanding_env': os.environ.get('NBLS_POOL_MAX_OUTSTANDING')}
    for mode in sys.argv[1:]:
        res[mode] = scenario(pkg, mode == 'balance', d1, d2, ref)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
