"""nbls_g2_combine_shares against the composition of the calls that existed before it, one JSON line: for the shapes groups x shares in {1 x 3, 8192 x 7, 1024 x 67, 64 x 667}
(valid signature shares of Shamir-split keys, made on the device) the median wall time, host clock around calls that end in a synchronisation, after warm-up, of
  (a) combine:     one nbls_g2_combine_shares call (Engine.combine_shares);
  (b) composition: Lagrange coefficients in Python integers, then decompress_batch, point_mul_batch, one point_sum call per group, compress_batch -- its host part (the
                   coefficients) is timed apart as well (b_host_lagrange);
  (c) lagrange:    nbls_lagrange_at_zero alone on the same identifiers (copies included): an upper bound of the Lagrange kernels' share of (a).
Both routes must give the same bytes.  The variants are interleaved (one call of each per round, the order rotated); min / max of every variant are recorded as its spread;
rocm-smi's shader clock and power are read right before and right after every shape and recorded beside its times (not while it runs).
Beside the shapes: nbls_lagrange_at_zero on ONE group of 65,536 identifiers, the largest group the calls accept (lagrange_1x65536; --no-big leaves it out).
--only-combine times (a) alone and checks nothing against (b): the form to put under rocprofv3 --kernel-trace --stats for the kernels' shares of the call.
usage: python tools/threshold_time.py [--reps R] [--out FILE] [--shapes 64x667,8192x7 ...] [--only-combine] [--no-big]"""
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
SHAPES = [(1, 3), (8192, 7), (1024, 67), (64, 667)]
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


def py_lagrange(ids):
    out = []
    for k, xk in enumerate(ids):
        num = den = 1
        for j, xj in enumerate(ids):
            if j != k:
                num = num * xj % R
                den = den * (xj - xk) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--only-combine', action='store_true')
    ap.add_argument('--no-big', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(667)
    res = {'tool': 'threshold_time', 'unit': 'ms', 'reps': a.reps, 'shapes': {}}
    host = {}

    def composition(groups):
        t = time.perf_counter()
        lam = [[v.to_bytes(32, 'big') for v in py_lagrange(ids)] for ids, _ in groups]
        host['ms'] = (time.perf_counter() - t) * 1e3
        aff, st = eng.decompress_batch(b''.join(s for _, sh in groups for s in sh), g2=True)
        assert not any(st)
        pts, st = eng.point_mul_batch([v for g in lam for v in g], aff, g2=True)
        assert not any(st)
        sums, at = [], 0
        for ids, _ in groups:
            p, z = eng.point_sum(pts[192 * at:192 * (at + len(ids))], g2=True)
            assert z == 0
            sums.append(p)
            at += len(ids)
        c = eng.compress_batch(b''.join(sums), g2=True)
        return [c[96 * g:96 * g + 96] for g in range(len(groups))]

    shapes = [tuple(int(v) for v in x.split('x')) for x in a.shapes.split(',')] if a.shapes else SHAPES
    for m, t in shapes:
        # four polynomials, cycled over the groups (the time does not depend on the values); every group signs its own message
        polys = []
        for _ in range(min(m, 4)):
            coef = [rnd.randrange(1, R) for _ in range(t)]
            ids = [rnd.randrange(1, R) for _ in range(t)]
            keys = []
            for x in ids:
                acc = 0
                for c in reversed(coef):
                    acc = (acc * x + c) % R
                keys.append(acc.to_bytes(32, 'big'))
            polys.append((ids, keys))
        msgs = [b'threshold %d of %d x %d' % (g, m, t) for g in range(m)]
        sigs = eng.sign_batch([msgs[g] for g in range(m) for _ in range(t)], [k for g in range(m) for k in polys[g % len(polys)][1]])
        groups = [(polys[g % len(polys)][0], sigs[g * t:(g + 1) * t]) for g in range(m)]
        variants = {'a_combine': lambda: eng.combine_shares(groups)[0], 'b_composition': lambda: composition(groups),
                    'c_lagrange_call': lambda: eng.lagrange_at_zero([ids for ids, _ in groups])}
        if a.only_combine:
            variants = {'a_combine': variants['a_combine']}
        want = variants['a_combine']()           # correct and warm
        if not a.only_combine:
            assert variants['b_composition']() == want
            variants['c_lagrange_call']()
        ts = {v: [] for v in variants}
        hosts, seq = [], []
        names = list(variants)
        before = smi()
        reps = {v: (min(a.reps, 3) if v == 'b_composition' and m * t * t > 10000000 else a.reps) for v in variants}   # Python's coefficients of 64 x 667 take seconds
        for r in range(a.reps):
            for v in names[r % len(names):] + names[:r % len(names)]:
                if len(ts[v]) >= reps[v]:
                    continue
                t0 = time.perf_counter()
                variants[v]()
                ts[v].append((time.perf_counter() - t0) * 1e3)
                seq.append([v[0], round(ts[v][-1], 2)])
                if v == 'b_composition':
                    hosts.append(host['ms'])
        after = smi()
        row = {v: round(statistics.median(x), 3) for v, x in ts.items()}
        row['spread_min_max'] = {v: [round(min(x), 3), round(max(x), 3)] for v, x in ts.items()}
        row['reps'] = {v: len(x) for v, x in ts.items()}
        if not a.only_combine:
            row['b_host_lagrange'] = round(statistics.median(hosts), 3)
            row['b_device_part'] = round(row['b_composition'] - row['b_host_lagrange'], 3)
            row['combine_over_composition'] = round(row['a_combine'] / row['b_composition'], 4)
            row['combine_over_composition_device_part'] = round(row['a_combine'] / row['b_device_part'], 4)
            row['lagrange_call_over_combine'] = round(row['c_lagrange_call'] / row['a_combine'], 4)
        row['sclk_power_before_after'] = [before, after]
        row['calls_in_order'] = seq             # [variant letter, ms] in the order they ran
        res['shapes']['%dx%d' % (m, t)] = row
        print(m, t, row, file=sys.stderr, flush=True)
    if not a.no_big and not a.only_combine:
        ids = [rnd.randrange(1, R) for _ in range(65536)]
        eng.lagrange_at_zero([ids])
        before, ts = smi(), []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.lagrange_at_zero([ids])
            ts.append(round((time.perf_counter() - t0) * 1e3, 1))
        res['lagrange_1x65536'] = {'calls': ts, 'sclk_power_before_after': [before, smi()]}
        print('1 x 65536', res['lagrange_1x65536'], file=sys.stderr, flush=True)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
