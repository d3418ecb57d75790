"""Times the PeerDAS recovery calls through the Python binding and writes profiles/kzg_recover.json.  No time is a pass condition.
  1 / 8 / 64 blobs at N = 4096 with cells of 64 elements (eight distinct random blobs, repeated: the device does the same work for a repeated blob), every blob from a random
  half of its 128 cells (indices shuffled), against a test-only monomial basis (kzg_cases.TAU)
  kzg_recover_cells, kzg_recover_cells_and_proofs; every result is checked against kzg_compute_cells_and_proofs on the original blobs, byte for byte
Each beside two things measured in the same run:
  python = the recovery in Python integers by the specification's route (kzg_recover_cases.recover) ON ONE blob, scaled to the call's size: the composition a caller has
           without these calls, for the field part alone
  compute = kzg_compute_cells / kzg_compute_cells_and_proofs on the same number of whole blobs: those calls are what they were before the recovery existed, so
           over_compute_ms = the call's median - theirs is what recovering costs over computing from a whole blob (for the proofs form: the front end; the proofs loop is shared)
Medians of `reps` calls after one warm-up call, min and max beside them; rocm-smi's shader clock and power are read right before and right after every shape.
--trace-workload: nothing is timed; `reps` calls of kzg_recover_cells and kzg_compute_cells on 64 blobs, of kzg_recover_cells on 8 and of kzg_recover_cells_and_proofs and
kzg_compute_cells_and_proofs on 8, for a kernel trace taken around the process (the kernels' own times are that trace's, not HIP events').
usage: python tools/kzg_recover_bench.py [--reps R] [--out FILE] [--blobs 1,8,64] [--trace-workload]"""
import argparse
import importlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kzg_cases import R, TAU, blob_bytes   # noqa: E402
from kzg_recover_cases import recover   # noqa: E402
from kzg_bench import smi, timed, g1   # noqa: E402

LOG2_N, LOG2_CELL = 12, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg_recover.json'))
    ap.add_argument('--blobs', default='1,8,64')
    ap.add_argument('--trace-workload', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2027)
    N, per, c = 1 << LOG2_N, 2 << (LOG2_N - LOG2_CELL), 1 << LOG2_CELL
    dblobs = [blob_bytes([rnd.randrange(R) for _ in range(N)]) for _ in range(8)]
    t, powers = 1, []
    for _ in range(N):
        powers.append(t)
        t = t * TAU % R
    su = eng.kzg_monomial_setup(LOG2_N, g1(eng, powers))
    dcells, st = eng.kzg_compute_cells(LOG2_N, LOG2_CELL, dblobs)
    assert st == bytes(8)

    def subset(n):
        idx = [rnd.sample(range(per), per // 2) for _ in range(n)]
        return idx, [[dcells[i % 8][k] for k in ks] for i, ks in enumerate(idx)]

    if a.trace_workload:
        idx64, given64 = subset(64)
        for _ in range(a.reps):
            eng.kzg_recover_cells(LOG2_N, LOG2_CELL, idx64, given64)
            eng.kzg_compute_cells(LOG2_N, LOG2_CELL, [dblobs[i % 8] for i in range(64)])
            eng.kzg_recover_cells(LOG2_N, LOG2_CELL, idx64[:8], given64[:8])
            eng.kzg_recover_cells_and_proofs(su, LOG2_CELL, idx64[:8], given64[:8])
            eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, dblobs)
        return
    res = {'reps': a.reps, 'log2_n': LOG2_N, 'log2_cell': LOG2_CELL, 'blobs': {}, 'what': __doc__.split('usage:')[0].strip()}
    ints = lambda cell: [int.from_bytes(cell[32 * j:32 * j + 32], 'big') for j in range(c)]
    idx1, given1 = subset(1)
    py = []
    res['python_recover_one_blob'] = timed(lambda: py.append(recover(idx1[0], [ints(x) for x in given1[0]], LOG2_N, LOG2_CELL)), 1)
    assert py[0][0] == 0 and py[0][1] == [ints(x) for x in dcells[0]]
    for n in [int(v) for v in a.blobs.split(',') if v]:
        blobs = [dblobs[i % 8] for i in range(n)]
        idx, given = subset(n)
        before = smi()
        want = eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs)
        assert eng.kzg_recover_cells_and_proofs(su, LOG2_CELL, idx, given) == want and want[2] == bytes(n)
        assert eng.kzg_recover_cells(LOG2_N, LOG2_CELL, idx, given) == (want[0], bytes(n))
        row = {'kzg_recover_cells': timed(lambda: eng.kzg_recover_cells(LOG2_N, LOG2_CELL, idx, given), a.reps),
               'kzg_compute_cells': timed(lambda: eng.kzg_compute_cells(LOG2_N, LOG2_CELL, blobs), a.reps),
               'kzg_recover_cells_and_proofs': timed(lambda: eng.kzg_recover_cells_and_proofs(su, LOG2_CELL, idx, given), a.reps),
               'kzg_compute_cells_and_proofs': timed(lambda: eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs), a.reps)}
        row['python_recover_scaled_ms'] = round(res['python_recover_one_blob']['median_ms'] * n, 3)
        row['cells_over_compute_ms'] = round(row['kzg_recover_cells']['median_ms'] - row['kzg_compute_cells']['median_ms'], 3)
        row['proofs_over_compute_ms'] = round(row['kzg_recover_cells_and_proofs']['median_ms'] - row['kzg_compute_cells_and_proofs']['median_ms'], 3)
        row['proofs_over_compute_share'] = round(row['proofs_over_compute_ms'] / row['kzg_compute_cells_and_proofs']['median_ms'], 4)
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
