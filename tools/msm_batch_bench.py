"""nbls_g*_msm_batch / nbls_g*_msm_rows against the composition of the calls that existed before them, one JSON line (profiles/msm_batch.json).  G1 shapes: rows 1000 x 667 and
groups x points 64 x 667, 1024 x 67, 8192 x 7, 1 x 65,536, with random 256-bit scalars and once more with 64-bit scalars; G2: 64 x 667 and 1024 x 67.  Per shape the median wall
time -- host clock around calls that end in a synchronisation, from host buffers through the Python binding, after warm-up -- of
  (a) batch:       one msm_batch / msm_rows call, window width automatic;
  (b) msm loop:    one nbls_g*_msm per group.  Every such call ends in a synchronisation, so above --sample groups (b) runs over a sample of the groups and is scaled to the
                   shape (b_msm_loop_scaled, the sample's size beside it): the cost per group does not depend on which groups are taken.  The sample's bytes must equal (a)'s;
  (c) ladders:     for groups of at most 7 points, one nbls_g1_mul_batch over all points (timed whole) and one nbls_g1_sum per group (the sums sampled and scaled like (b)):
                   c_ladders_scaled is their sum, batch_over_ladders the ratio;
  (w) the sweep:   (a) with NBLS_TUNE_MSMB_WINDOW forced to 4, 6, 8, 10, 12, and the width the automatic choice took (the argmin of its cost model, recomputed here).
All variants, the sweep included, are interleaved in one loop; min / max are recorded as the spread.  For the single-group shape the spread of the baseline itself comes from --spread-runs repeated blocks of
nbls_g*_msm calls (the medians of the blocks, min and max).  rocm-smi's shader clock and power are read right before and right after every shape.
usage: python tools/msm_batch_bench.py [--reps R] [--sample N] [--out FILE] [--only g1_256,g1_64,g2_256] [--no-sweep]"""
import argparse
import ctypes as C
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
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
G1_SHAPES = [('rows', 1000, 667), ('groups', 64, 667), ('groups', 1024, 67), ('groups', 8192, 7), ('groups', 1, 65536)]
G2_SHAPES = [('groups', 64, 667), ('groups', 1024, 67)]
WIDTHS = [4, 6, 8, 10, 12]


def smi():
    try:
        o = subprocess.run(['rocm-smi', '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20).stdout
        c = next(iter(json.loads(o).values()))
        sclk = [v for k, v in c.items() if 'sclk' in k.lower()]
        pw = [v for k, v in c.items() if 'power' in k.lower() and 'W' in k]
        return (sclk[0] if sclk else '?'), (pw[0] if pw else '?')
    except Exception as e:   # noqa: BLE001
        return '?', repr(e)[:40]


def auto_width(points_after_split, bits):
    cost = lambda c: points_after_split * -(-bits // c) + -(-bits // c) * c * (1 << (c - 1))
    return min(WIDTHS, key=lambda c: (cost(c), c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=32)
    ap.add_argument('--spread-runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default='g1_256,g1_64,g2_256')
    ap.add_argument('--no-sweep', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2026)
    res = {'tool': 'msm_batch_bench', 'unit': 'ms', 'reps': a.reps, 'sample': a.sample, 'shapes': {}}
    res['kernels'] = {n: eng.extra_program_kernel(n) for n in ('dbladd_g1', 'dbladd_g2')}
    # 4096 distinct points per group, cycled (the time does not depend on the values): [k]G, and [k]H(m) in G2 (sign is the engine's G2 ladder)
    keys = [rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(4096)]
    aff1, st = eng.point_mul_batch(keys)
    assert not any(st)
    aff2, st = eng.sign_batch_affine([b'msm_batch_bench'] * 512, keys[:512])
    assert not any(st)
    pool = {False: [aff1[96 * i:96 * i + 96] for i in range(4096)], True: [aff2[192 * i:192 * i + 192] for i in range(512)]}

    for run in a.only.split(','):
        g2, bits = run.startswith('g2'), int(run.split('_')[1])
        sz = 192 if g2 else 96
        msm = eng.lib.nbls_g2_msm if g2 else eng.lib.nbls_g1_msm
        for form, G, n in (G2_SHAPES if g2 else G1_SHAPES):
            pts_of = lambda g: b''.join(pool[g2][(g * 131 + j) % len(pool[g2])] for j in range(n))
            shared = pts_of(0)
            gpts = None if form == 'rows' else [pts_of(g) for g in range(G)]
            gks = [b''.join(rnd.getrandbits(bits).to_bytes(32, 'big') for _ in range(n)) for _ in range(G)]
            step = max(1, G // a.sample)
            sample = list(range(0, G, step))[:a.sample]
            scale = G / len(sample)

            def batch():
                return eng.msm_rows(shared, gks) if form == 'rows' else eng.msm_batch(gpts, gks, g2=g2)

            def one(g):
                out = C.create_string_buffer(sz); z = C.c_int8(0)
                assert msm(eng.h, n, shared if form == 'rows' else gpts[g], gks[g], out, C.byref(z)) == 0
                return out.raw, z.value

            def loop():
                return [one(g) for g in sample]

            small = n <= 7 and not g2
            allp = (shared * G if form == 'rows' else b''.join(gpts)) if small else None
            allk = [k[32 * i:32 * i + 32] for k in gks for i in range(n)] if small else None

            def ladder_muls():
                return eng.point_mul_batch(allk, allp)[0]

            def ladder_sums():
                return [eng.point_sum(prod[96 * n * g:96 * n * (g + 1)]) for g in sample]

            def forced(w):
                def f():
                    eng.set_msm_batch(window=w)
                    return batch()
                return f

            variants = {'a_batch': forced(0), 'b_msm_loop_sample': loop}
            if small:
                prod = ladder_muls()
                variants['c_ladder_muls'] = ladder_muls
                variants['c_ladder_sums_sample'] = ladder_sums
            sweep = [] if G == 1 or a.no_sweep else ['w%d' % w for w in WIDTHS]
            eng.set_msm_batch(window=0)
            got, gst = batch()                       # correct and warm
            assert [(got[g], gst[g]) for g in sample] == loop(), (run, form, G, n)
            for w in sweep:
                variants[w] = forced(int(w[1:]))
                assert variants[w]() == (got, gst), (run, form, G, n, w)
            ts = {v: [] for v in variants}
            names = list(variants)
            before = smi()
            for r in range(a.reps):
                for v in names[r % len(names):] + names[:r % len(names)]:
                    t0 = time.perf_counter()
                    variants[v]()
                    ts[v].append((time.perf_counter() - t0) * 1e3)
            eng.set_msm_batch(window=0)
            row = {v: round(statistics.median(x), 3) for v, x in ts.items() if v not in sweep}
            row['spread_min_max'] = {v: [round(min(x), 3), round(max(x), 3)] for v, x in ts.items()}
            row['sample_groups'] = len(sample)
            row['b_msm_loop_scaled'] = round(row['b_msm_loop_sample'] * scale, 3)
            row['batch_over_msm_loop'] = round(row['a_batch'] / row['b_msm_loop_scaled'], 4)
            if small:
                # the multiplications are one call over all points whatever the sample; only the sums scale
                row['c_ladders_scaled'] = round(row['c_ladder_muls'] + row['c_ladder_sums_sample'] * scale, 3)
                row['batch_over_ladders'] = round(row['a_batch'] / row['c_ladders_scaled'], 4)
            if sweep:
                row['window_sweep'] = {w[1:]: round(statistics.median(ts[w]), 3) for w in sweep}
            split = bits > 192
            row['auto_width'] = auto_width(n * ((4 if g2 else 2) if split else 1), (65 if g2 else 129) if split else bits) if G > 1 else 'single sum: the pipeline of msm'
            if G == 1:
                blocks = []
                for _ in range(a.spread_runs):
                    x = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter(); one(0); x.append((time.perf_counter() - t0) * 1e3)
                    blocks.append(statistics.median(x))
                row['baseline_block_medians'] = [round(b, 3) for b in blocks]
                row['baseline_run_to_run_spread'] = round(max(blocks) - min(blocks), 3)
            row['sclk_power_before_after'] = [before, smi()]
            res['shapes']['%s_%s_%dx%d' % (run, form, G, n)] = row
            print(run, form, G, n, row, file=sys.stderr, flush=True)
    res['config'] = eng.config_describe()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
