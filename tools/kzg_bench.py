"""Times nbls_kzg_verify_proofs and nbls_kzg_verify_blobs through the Python binding and writes profiles/kzg.json.  No time is a pass condition.
  proofs  64 / 4096 / 65,536 valid tuples (polynomials of four values, a test-only setup: the commitments and proofs are multiples of the generator made by get_public_keys)
  blobs   6 / 64 / 1024 blobs at N = 4096 (eight distinct blobs, repeated: the device does the same work for a repeated blob)
Each beside the composition of the older calls ON A SAMPLE, scaled to the call's size: decompress_batch of the 2 s points, fr_op for -y, point_mul_batch for [z]pi and [-y]G1, one
point_sum per item for C + [z]pi - [y]G1, pairing_batch of the 2 s pairs with the final exponentiation; for blobs also the Python-integer evaluation p(z) of the sample.  The host
cost of the challenges (SHA-256 of blob and commitment, inside nbls_kzg_verify_blobs) is measured beside them with hashlib on the same bytes.  Medians of `reps` calls after one
warm-up call, min and max beside them; rocm-smi's shader clock and power are read right before and right after every shape.
usage: python tools/kzg_bench.py [--reps R] [--sample S] [--out FILE] [--proofs 64,4096,65536] [--blobs 6,64,1024]"""
import argparse
import hashlib
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from kzg_cases import R, TAU, b32, eval_roots, blob_bytes, challenge   # noqa: E402


def smi():
    try:
        o = subprocess.run(['rocm-smi', '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20).stdout
        c = next(iter(json.loads(o).values()))
        sclk = [v for k, v in c.items() if 'sclk' in k.lower()]
        pw = [v for k, v in c.items() if 'power' in k.lower() and 'W' in k]
        return (sclk[0] if sclk else '?'), (pw[0] if pw else '?')
    except Exception as e:   # noqa: BLE001
        return '?', repr(e)[:40]


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(statistics.median(ts), 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3)}


def g1(eng, ks):
    """[k]G1 compressed for every k (0 -> the zero point's encoding)"""
    nz = [k for k in ks if k % R]
    pts = iter(eng.get_public_keys([b32(k % R) for k in nz])) if nz else iter(())
    return [next(pts) if k % R else b'\xc0' + bytes(47) for k in ks]


def composition(eng, cs, zs, ys, ps, tau_aff, g2_aff, reps):
    """the per-item check from the older calls, for the s items given"""
    s = len(cs)

    def run():
        aff, _ = eng.decompress_batch(b''.join(cs) + b''.join(ps))
        ny, _ = eng.fr_op('neg', ys)
        zp, _ = eng.point_mul_batch([b32(z) for z in zs], aff[96 * s:])
        yg, _ = eng.point_mul_batch(ny)
        xs = b''.join(eng.point_sum(aff[96 * i:96 * i + 96] + zp[96 * i:96 * i + 96] + yg[96 * i:96 * i + 96])[0] for i in range(s))
        eng.pairing_batch(aff[96 * s:] + xs, tau_aff * s + g2_aff * s, True, False)
    return timed(run, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg.json'))
    ap.add_argument('--proofs', default='64,4096,65536')
    ap.add_argument('--blobs', default='6,64,1024')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    import oracle_py
    oracle = oracle_py.load()
    eng = pkg.Engine(0)
    rnd = random.Random(2024)
    g2_aff = oracle.g2_generator()
    tau_aff = oracle.g2_mul(g2_aff, TAU)[1]
    tau_g2 = eng.compress_batch(tau_aff, g2=True)[:96]
    res = {'reps': a.reps, 'sample': a.sample, 'proofs': {}, 'blobs': {}, 'what': __doc__.split('usage:')[0].strip()}
    for n in [int(v) for v in a.proofs.split(',') if v]:
        fs = [[rnd.randrange(R) for _ in range(4)] for _ in range(n)]
        zs = [rnd.randrange(R) for _ in range(n)]
        pt = [eval_roots(f, TAU, 2) for f in fs]
        ys = [eval_roots(f, z, 2) for f, z in zip(fs, zs)]
        cs = g1(eng, pt)
        ps = g1(eng, [(p - y) * pow(TAU - z, -1, R) for p, y, z in zip(pt, ys, zs)])
        before = smi()
        ok, st = eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2)
        assert ok and st == bytes(n)
        row = {'kzg_verify_proofs': timed(lambda: eng.kzg_verify_proofs(cs, zs, ys, ps, tau_g2), a.reps)}
        bad = list(ys); bad[n // 2] = (ys[n // 2] + 1) % R
        row['kzg_verify_proofs_one_invalid_per_item_pass'] = timed(lambda: eng.kzg_verify_proofs(cs, zs, bad, ps, tau_g2), a.reps)
        s = min(n, a.sample)
        comp = composition(eng, cs[:s], zs[:s], ys[:s], ps[:s], tau_aff, g2_aff, a.reps)
        row['composition_sample'] = comp
        row['composition_sample_items'] = s
        row['composition_scaled_ms'] = round(comp['median_ms'] * n / s, 3)
        row['sclk_power_before_after'] = [before, smi()]
        res['proofs'][str(n)] = row
        print('proofs', n, row, file=sys.stderr, flush=True)
    log2_n = 12
    distinct = []
    for _ in range(8):
        f = [rnd.randrange(R) for _ in range(1 << log2_n)]
        blob = blob_bytes(f)
        pt = eval_roots(f, TAU, log2_n)
        c = g1(eng, [pt])[0]
        z = challenge(blob, c, log2_n)
        y = eval_roots(f, z, log2_n)
        distinct.append((f, blob, c, g1(eng, [(pt - y) * pow(TAU - z, -1, R)])[0], z, y))
    for n in [int(v) for v in a.blobs.split(',') if v]:
        items = [distinct[i % 8] for i in range(n)]
        blobs, cs, ps = [t[1] for t in items], [t[2] for t in items], [t[3] for t in items]
        before = smi()
        ok, st = eng.kzg_verify_blobs(log2_n, blobs, cs, ps, tau_g2)
        assert ok and st == bytes(n)
        row = {'kzg_verify_blobs': timed(lambda: eng.kzg_verify_blobs(log2_n, blobs, cs, ps, tau_g2), a.reps)}
        head = b'FSBLOBVERIFY_V1_' + (1 << log2_n).to_bytes(16, 'big')
        row['host_sha256_hashlib'] = timed(lambda: [hashlib.sha256(head + b + c).digest() for b, c in zip(blobs, cs)], a.reps)
        row['host_sha256_hashlib_ms_per_blob'] = round(row['host_sha256_hashlib']['median_ms'] / n, 4)
        s = min(n, 8, a.sample)
        row['python_eval_sample'] = timed(lambda: [eval_roots(t[0], t[4], log2_n) for t in items[:s]], 1)
        row['python_eval_scaled_ms'] = round(row['python_eval_sample']['median_ms'] * n / s, 3)
        comp = composition(eng, cs[:s], [t[4] for t in items[:s]], [t[5] for t in items[:s]], ps[:s], tau_aff, g2_aff, a.reps)
        row['composition_sample'] = comp
        row['composition_sample_items'] = s
        row['composition_scaled_ms'] = round((comp['median_ms'] + row['python_eval_sample']['median_ms']) * n / s, 3)
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
