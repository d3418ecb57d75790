"""nbls_verify_aggregates against today's composition, one JSON line: for the shapes sets x keys in {128 x 512, 1024 x 64, 4096 x 16, 65536 x 1} (65,536 distinct keys each
time, every set valid, signed on the device with the sum of its secret keys) the median wall time, host clock around calls that end in a synchronisation, after warm-up, of
  (a) per_call:    verify_aggregates, the compressed keys passed with the call (statuses requested: the combined check alone runs);
  (b) indexed:     verify_aggregates_indexed on a key table of the 65,536 keys made once before (the table's creation is timed apart: keyset_create_ms);
  (c) composition: today's route -- decompress_batch over every key, one g1_sum call per set, compress_batch of the sums, verify_multiple on the sets;
  (d) floor:       verify_multiple on n independent (signature, message, key) sets.
The variants are interleaved (one call of each per round, the order rotated); rocm-smi's shader clock and power are read right before and right after every shape and
recorded beside its times (not while it runs, so that the reads cannot disturb the calls).
usage: python tools/verify_aggregates_time.py [--reps R] [--out FILE]"""
import argparse
import importlib
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(128, 512), (1024, 64), (4096, 16), (65536, 1)]
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def smi():
    try:
        o = subprocess.run(['rocm-smi', '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20).stdout
        c = next(iter(json.loads(o).values()))
        sclk = [v for k, v in c.items() if 'sclk' in k.lower()]
        pw = [v for k, v in c.items() if 'power' in k.lower() and 'W' in k]
        return (sclk[0] if sclk else '?'), (pw[0] if pw else '?')
    except Exception as e:   # noqa: BLE001
        return '?', repr(e)[:40]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(5120)
    K = 65536
    sk = [rnd.randrange(1, R) for _ in range(K)]
    pks = eng.get_public_keys([k.to_bytes(32, 'big') for k in sk])
    t = time.perf_counter()
    table, st = eng.create_keyset(pks)
    res = {'tool': 'verify_aggregates_time', 'unit': 'ms', 'reps': a.reps, 'keys': K, 'keyset_create_ms': round((time.perf_counter() - t) * 1e3, 3), 'shapes': {}}
    assert st == bytes(K)

    def composition(sigs, msgs, sets):
        aff, kst = eng.decompress_batch(b''.join(b''.join(s) for s in sets))
        assert not any(kst)
        sums, at = [], 0
        for s in sets:
            p, z = eng.point_sum(aff[96 * at:96 * (at + len(s))])
            assert z == 0
            sums.append(p)
            at += len(s)
        agg = eng.compress_batch(b''.join(sums))
        return eng.verify_multiple(sigs, msgs, [agg[48 * j:48 * (j + 1)] for j in range(len(sets))])

    for n, k in SHAPES:
        msgs = [b'aggregate %d of %d x %d' % (j, n, k) for j in range(n)]
        sigs = eng.sign_batch(msgs, [(sum(sk[j * k:(j + 1) * k]) % R).to_bytes(32, 'big') for j in range(n)])
        sets = [pks[j * k:(j + 1) * k] for j in range(n)]
        idx = [list(range(j * k, (j + 1) * k)) for j in range(n)]
        fsigs = eng.sign_batch(msgs, [x.to_bytes(32, 'big') for x in sk[:n]])
        variants = {'a_per_call': lambda: eng.verify_aggregates(sigs, msgs, sets),
                    'b_indexed': lambda: eng.verify_aggregates_indexed(table, sigs, msgs, idx),
                    'c_composition': lambda: composition(sigs, msgs, sets),
                    'd_floor_verify_multiple': lambda: eng.verify_multiple(fsigs, msgs, pks[:n])}
        for f in variants.values():
            assert f() == (True, bytes(n))           # correct and warm
        reps = {v: (a.reps if v != 'c_composition' or n <= 4096 else 1) for v in variants}
        ts = {v: [] for v in variants}
        names = list(variants)
        seq = []
        before = smi()
        for r in range(a.reps):
            for v in names[r % len(names):] + names[:r % len(names)]:
                if len(ts[v]) < reps[v]:
                    t = time.perf_counter()
                    variants[v]()
                    ts[v].append((time.perf_counter() - t) * 1e3)
                    seq.append([v[0], round(ts[v][-1], 2)])
        after = smi()
        row = {v: round(statistics.median(x), 3) for v, x in ts.items()}
        row['reps'] = {v: len(x) for v, x in ts.items()}
        row['indexed_over_floor'] = round(row['b_indexed'] / row['d_floor_verify_multiple'], 3)
        row['per_call_over_composition'] = round(row['a_per_call'] / row['c_composition'], 4)
        row['sclk_power_before_after'] = [before, after]
        row['calls_in_order'] = seq             # [variant letter, ms] in the order they ran
        res['shapes']['%dx%d' % (n, k)] = row
        print(n, k, row, file=sys.stderr, flush=True)
    table.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
