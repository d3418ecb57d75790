"""The shared-message calls against the existing entry points on the expanded input, one JSON line.  Shapes n sets x m messages: 4096 x 4096 (identity index), 4096 x 64,
65,536 x 65,536, 65,536 x 1024, 65,536 x 64, 65,536 x 1 through verify_multiple_shared / verify_multiple, and 1024 sets x 64 keys over 16 messages through
verify_aggregates_indexed_shared / verify_aggregates_indexed on a key table of 65,536 keys.  Every set is valid and signed on the device; set i signs message i mod m (the index is passed as a numpy uint32 array).  Per
shape the median wall time, host clock around calls that end in a synchronisation, after warm-up, of
  (a) shared:   the shared-message call on the m distinct messages and the index;
  (b) expanded: the existing entry point, every set given the bytes of its message.
The variants are interleaved (one call of each per round, the order rotated); rocm-smi's shader clock and power are read right before and right after every shape and recorded
beside its times (not while it runs, so that the reads cannot disturb the calls); every call's time is kept in the order the calls ran.
usage: python tools/verify_shared_time.py [--reps R] [--out FILE] [--shapes 4096x64,65536x1 ...] [--no-aggregates]"""
import argparse
import importlib
import json
import os
import random
import statistics
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (4096, 64), (65536, 65536), (65536, 1024), (65536, 64), (65536, 1)]
AGG = (1024, 64, 16)     # sets, keys per set, messages
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


def measure(variants, n, reps):
    for f in variants.values():
        assert f() == (True, bytes(n))           # correct and warm
    ts = {v: [] for v in variants}
    names = list(variants)
    seq = []
    before = smi()
    for r in range(reps):
        for v in names[r % len(names):] + names[:r % len(names)]:
            t = time.perf_counter()
            variants[v]()
            ts[v].append((time.perf_counter() - t) * 1e3)
            seq.append([v[0], round(ts[v][-1], 2)])
    after = smi()
    row = {v: round(statistics.median(x), 3) for v, x in ts.items()}
    row['min_max'] = {v: [round(min(x), 3), round(max(x), 3)] for v, x in ts.items()}
    row['shared_over_expanded'] = round(row['a_shared'] / row['b_expanded'], 4)
    row['sclk_power_before_after'] = [before, after]
    row['calls_in_order'] = seq             # [variant letter, ms] in the order they ran
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--no-aggregates', action='store_true')
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split('x')) for s in a.shapes.split(',')] if a.shapes else SHAPES
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(6400)
    K = 65536
    sk = [rnd.randrange(1, R) for _ in range(K)]
    raw = [k.to_bytes(32, 'big') for k in sk]
    pks = eng.get_public_keys(raw)
    res = {'tool': 'verify_shared_time', 'unit': 'ms', 'reps': a.reps, 'shapes': {}}
    for n, m in shapes:
        msgs = [b'signing root %d of %d x %d' % (g, n, m) for g in range(m)]
        index = np.arange(n, dtype=np.uint32) % np.uint32(m)      # a uint32 array goes to the library without a copy (a list of 65,536 ints costs the binding ~3 ms)
        full = [msgs[g] for g in index.tolist()]
        sigs = eng.sign_batch(full, raw[:n])
        row = measure({'a_shared': lambda: eng.verify_multiple_shared(sigs, msgs, index, pks[:n]),
                       'b_expanded': lambda: eng.verify_multiple(sigs, full, pks[:n])}, n, a.reps)
        res['shapes']['%dx%d' % (n, m)] = row
        print(n, m, {k: v for k, v in row.items() if k != 'calls_in_order'}, file=sys.stderr, flush=True)
    if not a.no_aggregates:
        n, k, m = AGG
        table, st = eng.create_keyset(pks)
        assert st == bytes(K)
        msgs = [b'aggregate root %d' % g for g in range(m)]
        index = np.arange(n, dtype=np.uint32) % np.uint32(m)
        full = [msgs[g] for g in index.tolist()]
        idx = [list(range(j * k, (j + 1) * k)) for j in range(n)]
        sigs = eng.sign_batch(full, [(sum(sk[j * k:(j + 1) * k]) % R).to_bytes(32, 'big') for j in range(n)])
        row = measure({'a_shared': lambda: eng.verify_aggregates_indexed_shared(table, sigs, msgs, index, idx),
                       'b_expanded': lambda: eng.verify_aggregates_indexed(table, sigs, full, idx)}, n, a.reps)
        res['shapes']['indexed_%dx%d_over_%d' % (n, k, m)] = row
        print('indexed', n, k, m, {k_: v for k_, v in row.items() if k_ != 'calls_in_order'}, file=sys.stderr, flush=True)
        table.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
