"""Times the KZG prover's calls through the Python binding and writes profiles/kzg_prove.json.  No time is a pass condition.
  6 / 64 / 1024 blobs at N = 4096 (eight distinct random blobs, repeated: the device does the same work for a repeated blob), against a test-only setup (kzg_cases.TAU)
  kzg_commit_blobs, kzg_compute_proofs, kzg_compute_blob_proofs with the commitments given and with none; every result of the first shape is checked against the composition
Each beside the composition of the calls that existed before them:
  commitment = msm_rows over the setup's affine points kept on the host (decoded and split again on every call) + compress_batch
  proof      = fr_eval_roots for y, the quotient in Python integers ON A SAMPLE of blobs scaled to the call's size (kzg_prove_cases.quotient: one batch inversion per blob, cheaper
               than 4096 modular divisions), msm_rows, compress_batch
and beside fr_quotient_roots / fr_eval_roots at the same n (both with their copies: the quotient reads 32 N bytes per polynomial back, the evaluation 32).  Medians of `reps` calls
after one warm-up call, min and max beside them; rocm-smi's shader clock and power are read right before and right after every shape.
usage: python tools/kzg_prove_bench.py [--reps R] [--sample S] [--out FILE] [--blobs 6,64,1024]"""
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
from kzg_cases import R, TAU, b32, roots, blob_bytes   # noqa: E402
from kzg_prove_cases import quotient   # noqa: E402
from kzg_bench import smi, timed, g1   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg_prove.json'))
    ap.add_argument('--blobs', default='6,64,1024')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2025)
    log2_n = 12
    N, w = 1 << log2_n, roots(log2_n)
    fac = (pow(TAU, N, R) - 1) * pow(N, -1, R) % R
    lag48 = g1(eng, [fac * wj % R * pow(TAU - wj, -1, R) for wj in w])
    lag_aff, st = eng.decompress_batch(b''.join(lag48))
    assert not any(st)
    res = {'reps': a.reps, 'sample': a.sample, 'log2_n': log2_n, 'blobs': {}, 'what': __doc__.split('usage:')[0].strip()}
    res['kzg_setup_create'] = timed(lambda: eng.kzg_setup(log2_n, lag48).close(), a.reps)
    su = eng.kzg_setup(log2_n, lag48)
    distinct = [[rnd.randrange(R) for _ in range(N)] for _ in range(8)]
    dblobs = [blob_bytes(f) for f in distinct]
    dz = [rnd.randrange(R) for _ in range(8)]
    for n in [int(v) for v in a.blobs.split(',') if v]:
        blobs, zs = [dblobs[i % 8] for i in range(n)], [dz[i % 8] for i in range(n)]
        before = smi()
        cs, st = eng.kzg_commit_blobs(su, blobs)
        assert st == bytes(n)
        row = {'kzg_commit_blobs': timed(lambda: eng.kzg_commit_blobs(su, blobs), a.reps)}
        row['kzg_compute_proofs'] = timed(lambda: eng.kzg_compute_proofs(su, blobs, zs), a.reps)
        row['kzg_compute_blob_proofs_given_commitments'] = timed(lambda: eng.kzg_compute_blob_proofs(su, blobs, cs), a.reps)
        row['kzg_compute_blob_proofs_no_commitments'] = timed(lambda: eng.kzg_compute_blob_proofs(su, blobs), a.reps)
        row['fr_eval_roots'] = timed(lambda: eng.fr_eval_roots(log2_n, b''.join(blobs), zs), a.reps)
        if n <= 64:      # (the binding slices 4096 values per polynomial out of the read-back: not a time of the call at 1024)
            row['fr_quotient_roots'] = timed(lambda: eng.fr_quotient_roots(log2_n, b''.join(blobs), zs), a.reps)

        def commit_composed(rows):
            aff, zero = eng.msm_rows(lag_aff, rows)
            return eng.compress_batch(b''.join(aff)), zero
        row['composition_commit'] = timed(lambda: commit_composed(blobs), a.reps)
        s = min(n, a.sample)
        qrows = []

        def py_quotients():
            qrows[:] = [b''.join(b32(v) for v in quotient(distinct[i % 8], zs[i], log2_n)[1]) for i in range(s)]
        row['python_quotient_sample'] = timed(py_quotients, 1)
        row['python_quotient_sample_blobs'] = s
        row['python_quotient_scaled_ms'] = round(row['python_quotient_sample']['median_ms'] * n / s, 3)
        allq = [qrows[i % s] for i in range(n)]      # (rows of the right shape for the MSM's time; only the first s are the blobs' own)
        row['composition_proof_device_part'] = timed(lambda: (eng.fr_eval_roots(log2_n, b''.join(blobs), zs), commit_composed(allq)), a.reps)
        row['composition_proof_scaled_ms'] = round(row['composition_proof_device_part']['median_ms'] + row['python_quotient_scaled_ms'], 3)
        if n == int(a.blobs.split(',')[0]):      # the two routes agree, byte for byte
            assert commit_composed(blobs)[0] == b''.join(cs)
            ps, ys, _ = eng.kzg_compute_proofs(su, blobs, zs)
            assert commit_composed(qrows)[0] == b''.join(ps[:s]) and ys == eng.fr_eval_roots(log2_n, b''.join(blobs), zs)[0]
            assert eng.kzg_compute_blob_proofs(su, blobs)[0] == cs
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
