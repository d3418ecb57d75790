"""nbls_verify_multiple against today's routes, one JSON line: for n in {1, 64, 1024, 4096, 16384, 65536} sets (distinct keys and messages, signed on the device) the median
wall time, host clock around calls that end in a synchronisation, after warm-up, of
  (a) verify_multiple, every set valid (statuses requested: the combined check alone runs);
  (b) verify_multiple with one invalid set (the last), statuses requested: the combined check plus the per-set pass;
  (c) verify_batch at the same n (one aggregate signature over n messages), the floor;
  (d) for n <= 1024: n sequential verify calls (nbls_verify_batch with n = 1), today's route for independent sets.
usage: python tools/verify_multiple_time.py [--reps R] [--out FILE]"""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [1, 64, 1024, 4096, 16384, 65536]
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(4242)
    N = max(SIZES)
    sks = [rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(N)]
    msgs = [b'set %d ' % i + rnd.getrandbits(64).to_bytes(8, 'big') for i in range(N)]
    sigs = eng.sign_batch(msgs, sks)
    pks = eng.get_public_keys(sks)
    res = {'tool': 'verify_multiple_time', 'unit': 'ms', 'reps': a.reps, 'sizes': {}}
    for n in SIZES:
        S, M, P = sigs[:n], msgs[:n], pks[:n]
        ok, _ = eng.verify_multiple(S, M, P)
        assert ok
        bad = list(M); bad[-1] = bad[-1] + b'!'
        ok, st = eng.verify_multiple(S, bad, P)
        assert not ok and st[-1] == 9 and not any(st[:-1])
        reps = a.reps if n <= 16384 else max(3, a.reps // 2)
        row = {'a_all_valid': timed(lambda: eng.verify_multiple(S, M, P), reps),
               'b_one_invalid_per_set': timed(lambda: eng.verify_multiple(S, bad, P), reps),
               'c_verify_batch': timed(lambda: eng.verify_batch(S[0], M, P), reps)}
        if n <= 1024:
            row['d_sequential_verify'] = timed(lambda: [eng.verify_batch(S[i], [M[i]], [P[i]]) for i in range(n)], max(3, reps // 2), warm=1)
        row['b_minus_a'] = round(row['b_one_invalid_per_set'] - row['a_all_valid'], 3)
        res['sizes'][str(n)] = row
        print(n, row, file=sys.stderr, flush=True)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
