"""Times the PeerDAS calls through the Python binding and writes profiles/kzg_cells.json.  No time is a pass condition.
  1 / 8 / 64 blobs at N = 4096 with cells of 64 elements (eight distinct random blobs, repeated: the device does the same work for a repeated blob), against a test-only
  monomial basis (kzg_cases.TAU)
  kzg_compute_cells, kzg_compute_cells_and_proofs; every result of the first shape is checked against the composition
Each beside the composition of what existed before them:
  cells  = the transform in Python integers (kzg_cells_cases.cells) ON A SAMPLE of blobs, scaled to the call's size
  proofs = the coefficients and the 128 quotient rows of a blob in Python integers ON A SAMPLE of blobs, scaled; then msm_rows of the rows over the basis' affine points kept on
           the host (decoded and split again on every call) + compress_batch, run for at most 8 blobs (one pass of the batched MSM: 2^22 scalars) and scaled to the call's size
and beside msm_rows alone over the same rows x points: share_not_msm = 1 - that time / the call's.  (It can come out negative: msm_rows sends its scalars, 128 KB per
row, from the host, which the call's rows never cross; the kernel trace separates the kernels.)  Medians of `reps` calls after one warm-up call, min and max beside them; rocm-smi's shader clock and power are read right before and right after every shape.
--trace-workload: nothing is timed; `reps` calls of fr_ntt in both directions and of kzg_compute_cells on 1024 polynomials of 4096 elements, and of
kzg_compute_cells_and_proofs on 8 blobs, for a kernel trace taken around the process (the kernels' own times are that trace's, not HIP events').
usage: python tools/kzg_cells_bench.py [--reps R] [--sample S] [--out FILE] [--blobs 1,8,64] [--trace-workload]"""
import argparse
import ctypes as C
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
from kzg_cells_cases import cells, to_coeffs, cell_quotient, rows   # noqa: E402
from kzg_bench import smi, timed, g1   # noqa: E402

LOG2_N, LOG2_CELL = 12, 6
PER_PASS = 8      # mainnet blobs in one pass of the batched MSM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg_cells.json'))
    ap.add_argument('--blobs', default='1,8,64')
    ap.add_argument('--trace-workload', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2026)
    N, per = 1 << LOG2_N, 2 << (LOG2_N - LOG2_CELL)
    distinct = [[rnd.randrange(R) for _ in range(N)] for _ in range(8)]
    dblobs = [blob_bytes(f) for f in distinct]
    t, powers = 1, []
    for _ in range(N):
        powers.append(t)
        t = t * TAU % R
    mono48 = g1(eng, powers)
    if a.trace_workload:
        polys = b''.join(dblobs[i % 8] for i in range(1024))
        out = C.create_string_buffer(len(polys))
        su = eng.kzg_monomial_setup(LOG2_N, mono48)
        for _ in range(a.reps):
            for d in (0, 1):      # (the raw call: the binding's slicing of 4 M values is no part of the trace's subject)
                assert eng.lib.nbls_fr_ntt(eng.h, LOG2_N, d, 1024, polys, None, out, None) == 0
            eng.kzg_compute_cells(LOG2_N, LOG2_CELL, [dblobs[i % 8] for i in range(1024)])
            eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, dblobs)
        return
    mono_aff, st = eng.decompress_batch(b''.join(mono48))
    assert not any(st)
    res = {'reps': a.reps, 'sample': a.sample, 'log2_n': LOG2_N, 'log2_cell': LOG2_CELL, 'blobs': {}, 'what': __doc__.split('usage:')[0].strip()}
    res['kzg_monomial_setup'] = timed(lambda: eng.kzg_monomial_setup(LOG2_N, mono48).close(), a.reps)
    su = eng.kzg_monomial_setup(LOG2_N, mono48)

    def rows_composed(qrows):
        aff, zero = eng.msm_rows(mono_aff, qrows)
        return eng.compress_batch(b''.join(aff)), zero

    for n in [int(v) for v in a.blobs.split(',') if v]:
        blobs = [dblobs[i % 8] for i in range(n)]
        before = smi()
        got_cells, got_proofs, st = eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs)
        assert st == bytes(n)
        row = {'kzg_compute_cells': timed(lambda: eng.kzg_compute_cells(LOG2_N, LOG2_CELL, blobs), a.reps)}
        row['kzg_compute_cells_and_proofs'] = timed(lambda: eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, blobs), a.reps)
        s = min(n, a.sample)
        py_cells, qrows = [], []

        def python_cells():
            py_cells[:] = [cells(distinct[i % 8], LOG2_N, LOG2_CELL) for i in range(s)]

        def python_rows():
            qrows[:] = []
            for i in range(s):
                coef = to_coeffs(distinct[i % 8], LOG2_N)
                qrows.extend(rows(cell_quotient(coef, k, LOG2_N, LOG2_CELL)) for k in range(per))
        row['python_cells_sample'] = timed(python_cells, 1)
        row['python_rows_sample'] = timed(python_rows, 1)
        row['python_sample_blobs'] = s
        row['composition_cells_scaled_ms'] = round(row['python_cells_sample']['median_ms'] * n / s, 3)
        m = min(n, PER_PASS)      # blobs of one msm_rows call
        allq = [qrows[i % len(qrows)] for i in range(m * per)]      # (rows of the right shape for the MSM's time; only the first s * 128 are the blobs' own)
        row['msm_rows_blobs'] = m
        row['msm_rows_and_compress'] = timed(lambda: rows_composed(allq), a.reps)
        row['msm_rows_alone'] = timed(lambda: eng.msm_rows(mono_aff, allq), a.reps)
        row['composition_proofs_scaled_ms'] = round(row['python_rows_sample']['median_ms'] * n / s + row['msm_rows_and_compress']['median_ms'] * n / m, 3)
        row['msm_rows_alone_scaled_ms'] = round(row['msm_rows_alone']['median_ms'] * n / m, 3)
        row['share_not_msm'] = round(1 - row['msm_rows_alone_scaled_ms'] / row['kzg_compute_cells_and_proofs']['median_ms'], 4)
        if n == int(a.blobs.split(',')[0]):      # the two routes agree, byte for byte
            for i in range(s):
                assert [[int.from_bytes(c[32 * j:32 * j + 32], 'big') for j in range(1 << LOG2_CELL)] for c in got_cells[i]] == py_cells[i]
            assert rows_composed(qrows)[0] == b''.join(p for ps in got_proofs[:s] for p in ps)
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
