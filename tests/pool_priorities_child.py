"""Child process of tests/test_gpu_pool_priorities.py: the HIP runtime reads GPU_MAX_HW_QUEUES once, when it initialises, so every case runs in a process of its own
with the variable as the parent set it.  argv: MODE DEPTH, MODE = ex (nbls_pool_init_ex with NBLS_POOL_SPREAD_PRIORITIES) or plain (nbls_pool_init).  Prints one JSON line:
the stream priority of every context, the device's priority range, and -- mode ex, depth 12 -- how many outputs of three rounds of submits with n = 7 and n = 257 differ from
a one-context nbls_pairing_batch_dev and from the oracle."""
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    mode, depth = sys.argv[1], int(sys.argv[2])
    pkg = importlib.import_module('noble-bls12-381_amd')
    torch.cuda.init()
    # the range as HIP reports it (torch.cuda.Stream.priority_range() clamps it to two levels), asked of the runtime this process has loaded
    hip = C.CDLL(next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line))
    lo, hi = C.c_int(), C.c_int()
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(lo), C.byref(hi)) == 0
    least, greatest = lo.value, hi.value
    res = {'queues': os.environ.get('GPU_MAX_HW_QUEUES'), 'priority_range': [least, greatest], 'levels': least - greatest + 1}
    if mode == 'plain':
        lib = pkg.engine.load_library()
        h = C.c_void_p()
        assert lib.nbls_pool_init(0, depth, C.byref(h)) == 0
        prios = []
        for i in range(depth):
            v = C.c_int(99)
            assert lib.nbls_pool_stream_priority(h, i, C.byref(v)) == 0
            prios.append(v.value)
        v = C.c_int()
        res['bad_index'] = [lib.nbls_pool_stream_priority(h, -1, C.byref(v)), lib.nbls_pool_stream_priority(h, depth, C.byref(v))]
        lib.nbls_pool_destroy(h)
        res['priorities'] = prios
        print(json.dumps(res), flush=True)
        return
    pipe = pkg.PairingPipeline(0, depth)      # spread_priorities=True is the default
    res['priorities'] = pipe.stream_priorities()
    if depth == 12:
        import bench
        import oracle_py
        oracle = oracle_py.load()
        N = 257      # 7 and 257: a ragged last wavefront for both item layouts of the step kernels (10 x 6 and 12 x 5 items a wavefront)
        G1, G2 = bench.synth_stream(pipe.engines[0], oracle, N, seed=0x7072696f)
        ref, _ = oracle.pairing_batch(G1, G2, True, False, threads=min(16, os.cpu_count() or 8))
        d1 = torch.frombuffer(bytearray(G1), dtype=torch.uint8).cuda(); d2 = torch.frombuffer(bytearray(G2), dtype=torch.uint8).cuda()
        single = pkg.Engine(0)
        one = torch.zeros(576 * N, dtype=torch.uint8, device='cuda')
        res['differ_from_single'] = 0; res['differ_from_oracle'] = 0; res['compared'] = 0
        for n in (7, N):      # item i of the stream does not depend on n: the first 7 pairs are the n = 7 case
            one.zero_()
            single.pairing_batch_dev(n, d1.data_ptr(), d2.data_ptr(), one.data_ptr(), True, None)
            torch.cuda.synchronize()
            want = bytes(one[:576 * n].cpu().numpy().tobytes())
            res['differ_from_oracle'] += int(want != ref[:576 * n])
            outs = [torch.zeros(576 * n, dtype=torch.uint8, device='cuda') for _ in range(depth)]
            for rnd in range(3):      # three rounds over the contexts, all in flight together
                for _ in range(depth):
                    pipe.submit(n, d1.data_ptr(), d2.data_ptr(), outs[pipe.slot].data_ptr(), True)
            pipe.synchronize()
            for o in outs:
                got = bytes(o.cpu().numpy().tobytes())
                res['compared'] += 1
                res['differ_from_single'] += int(got != want)
                res['differ_from_oracle'] += int(got != ref[:576 * n])
        single.close()
    pipe.close()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
