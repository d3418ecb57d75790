"""Times the FK20 cell-proof calls beside the calls they must equal, through the Python binding, and writes profiles/kzg_fk20.json.  No time is a pass condition.
  1 / 8 / 64 blobs at N = 4096 with cells of 64 elements (eight distinct random blobs, repeated), against a test-only monomial basis (kzg_cases.TAU)
  kzg_compute_cells_and_proofs_fk20 and kzg_compute_cells_and_proofs INTERLEAVED in the same run on the same blobs: one warm-up call of each, then `reps` rounds of one
  call of each, the FK20 call first in even rounds and second in odd ones; the recovery pair likewise, every blob from a random half of its cells
  ratio = the other call's median / the FK20 call's median; spread = (max - min) / median of each
  the results of the two calls are compared once per shape, byte for byte
  kzg_fk20_setup is timed once (the handle's one batched MSM and its two kernels)
rocm-smi's shader clock and power are read right before and right after every shape.
--trace-workload: nothing is timed; `reps` FK20 calls on 8 blobs for a kernel trace taken around the process (the scalars kernel, pass A, the conversion and pass B are
told apart by their kernels there).
usage: python tools/kzg_fk20_bench.py [--reps R] [--out FILE] [--blobs 1,8,64] [--trace-workload]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kzg_cases import R, TAU, blob_bytes   # noqa: E402
from kzg_bench import smi, g1   # noqa: E402

LOG2_N, LOG2_CELL = 12, 6


def stats(ts):
    med = statistics.median(ts)
    return {'median_ms': round(med, 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3), 'spread': round((max(ts) - min(ts)) / med, 4)}


def interleaved(new, old, reps):
    """one warm-up call of each, then `reps` rounds of one call of each in alternating order -> (stats of new, stats of old, old's median / new's)"""
    new(); old()
    tn, to = [], []
    for k in range(reps):
        for f, ts in ((new, tn), (old, to)) if k % 2 == 0 else ((old, to), (new, tn)):
            t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    a, b = stats(tn), stats(to)
    return a, b, round(b['median_ms'] / a['median_ms'], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg_fk20.json'))
    ap.add_argument('--blobs', default='1,8,64')
    ap.add_argument('--trace-workload', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2027)
    N, per = 1 << LOG2_N, 2 << (LOG2_N - LOG2_CELL)
    dblobs = [blob_bytes([rnd.randrange(R) for _ in range(N)]) for _ in range(8)]
    t, powers = 1, []
    for _ in range(N):
        powers.append(t)
        t = t * TAU % R
    su = eng.kzg_monomial_setup(LOG2_N, g1(eng, powers))
    if a.trace_workload:
        fk = eng.kzg_fk20_setup(su, LOG2_CELL)
        for _ in range(a.reps):
            eng.kzg_compute_cells_and_proofs_fk20(fk, dblobs)
        return
    res = {'reps': a.reps, 'log2_n': LOG2_N, 'log2_cell': LOG2_CELL, 'blobs': {}, 'what': __doc__.split('usage:')[0].strip()}
    t0 = time.perf_counter()
    fk = eng.kzg_fk20_setup(su, LOG2_CELL)
    res['kzg_fk20_setup_ms'] = round((time.perf_counter() - t0) * 1e3, 3)
    for n in [int(v) for v in a.blobs.split(',') if v]:
        blobs = [dblobs[i % 8] for i in range(n)]
        before = smi()
        want = eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs)
        assert eng.kzg_compute_cells_and_proofs_fk20(fk, blobs) == want and want[2] == bytes(n)
        idxs = [rnd.sample(range(per), per // 2) for _ in range(n)]
        given = [[want[0][i][k] for k in idx] for i, idx in enumerate(idxs)]
        assert eng.kzg_recover_cells_and_proofs_fk20(fk, idxs, given) == eng.kzg_recover_cells_and_proofs(su, LOG2_CELL, idxs, given) == want
        row = {}
        row['compute_fk20'], row['compute'], row['compute_ratio'] = interleaved(lambda: eng.kzg_compute_cells_and_proofs_fk20(fk, blobs),
                                                                               lambda: eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs), a.reps)
        row['recover_fk20'], row['recover'], row['recover_ratio'] = interleaved(lambda: eng.kzg_recover_cells_and_proofs_fk20(fk, idxs, given),
                                                                               lambda: eng.kzg_recover_cells_and_proofs(su, LOG2_CELL, idxs, given), a.reps)
        row['sclk_power_before_after'] = [before, smi()]
        res['blobs'][str(n)] = row
        print('blobs', n, row, file=sys.stderr, flush=True)
    res['config'] = eng.config_describe()
    print(json.dumps(res, sort_keys=True))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
