"""nbls_g1_poly_eval / nbls_g2_poly_eval against the composition of the calls that existed before them, one JSON line (profiles/poly_eval.json).  For the shapes
groups x (t coefficients, m identifiers) in {1 x (3, 5), 8192 x (5, 7), 1024 x (67, 100), 1 x (667, 1000)}, in G1 and G2, once with the identifiers 1 .. m (the 16-bit form of the
Horner step) and once with random 256-bit identifiers (the 256-bit form), the median wall time -- host clock around calls that end in a synchronisation, after warm-up -- of
  (a) poly_eval:    one nbls_g*_poly_eval call (Engine.poly_eval);
  (b) composition:  the powers x^j mod r in Python integers, one decompress_batch of the coefficients, one nbls_g*_msm per identifier, one compress_batch.  Its host part (the
                    powers) is timed apart (b_host_powers).  A shape has up to 102,400 identifiers and every msm call ends in a synchronisation, so (b) runs over a SAMPLE of
                    at most --sample identifiers spread over the groups and is scaled to the shape (b_composition_scaled, the sample's size beside it): the cost per identifier
                    does not depend on which identifiers are taken.  The sample's bytes must equal (a)'s.
The variants are interleaved; min / max are recorded as the spread; rocm-smi's shader clock and power are read right before and right after every shape.
--force-full and NBLS_AOT=0 in the environment give the two A/B runs the record needs: the 256-bit form on the identifiers 1 .. m (the call is widened by one more group of one
coefficient and the identifier 2^16, which the record says) and the interpreter in place of the ahead-of-time kernels.  nbls_config_describe() is part of the record.
usage: python tools/poly_time.py [--reps R] [--out FILE] [--shapes 1x3x5,8192x5x7 ...] [--sides g1,g2] [--sample N] [--only-eval] [--force-full]"""
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
SHAPES = [(1, 3, 5), (8192, 5, 7), (1024, 67, 100), (1, 667, 1000)]
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
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--sides', default='g1,g2')
    ap.add_argument('--sample', type=int, default=64)
    ap.add_argument('--only-eval', action='store_true')
    ap.add_argument('--force-full', action='store_true', help='the 256-bit form on the short identifiers too: one more group of one coefficient and the identifier 2^16')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(1000)
    res = {'tool': 'poly_time', 'unit': 'ms', 'reps': a.reps, 'sample': a.sample, 'force_full': a.force_full, 'shapes': {}}
    res['kernels'] = {n: eng.extra_program_kernel(n) for n in ('poly_g1_16', 'poly_g1_256', 'poly_g2_16', 'poly_g2_256')}
    shapes = [tuple(int(v) for v in x.split('x')) for x in a.shapes.split(',')] if a.shapes else SHAPES
    host = {}
    for side in a.sides.split(','):
        g2 = side == 'g2'
        e = 96 if g2 else 48

        def commit(keys):
            # [a_j]G in G1; in G2 [a_j]H(m), a commitment to the same polynomial on another base (sign is the engine's G2 ladder)
            return eng.sign_batch([b'poly_time'] * len(keys), keys) if g2 else eng.get_public_keys(keys)

        for G, t, m in shapes:
            # four polynomials, cycled over the groups (the time does not depend on the values)
            polys = [commit([rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(t)]) for _ in range(min(G, 4))]
            for form in ('short', 'full'):
                ids = [list(range(1, m + 1)) if form == 'short' else [rnd.getrandbits(256) for _ in range(m)] for _ in range(min(G, 4))]
                groups = [(polys[g % len(polys)], ids[g % len(ids)]) for g in range(G)]
                if a.force_full and form == 'short':
                    groups.append((polys[0][:1], [1 << 16]))
                total = G * m
                step = max(1, total // a.sample)
                sample = list(range(0, total, step))[:a.sample]

                def composition():
                    t0 = time.perf_counter()
                    pw = []
                    for k in sample:
                        x, v, row = groups[k // m][1][k % m] % R, 1, []
                        for _ in range(t):
                            row.append(v.to_bytes(32, 'big'))
                            v = v * x % R
                        pw.append(row)
                    host['ms'] = (time.perf_counter() - t0) * 1e3
                    which = sorted(set((k // m) % len(polys) for k in sample))
                    aff, st = eng.decompress_batch(b''.join(c for p in which for c in polys[p]), g2=g2)
                    assert not any(st)
                    a2 = 2 * e
                    pts = {p: aff[i * t * a2:(i + 1) * t * a2] for i, p in enumerate(which)}
                    out = b''
                    for k, row in zip(sample, pw):
                        p, z = eng.msm(pts[(k // m) % len(polys)], row, g2=g2)
                        assert z == 0
                        out += p
                    c = eng.compress_batch(out, g2=g2)
                    return [c[e * i:e * i + e] for i in range(len(sample))]

                variants = {'a_poly_eval': lambda: eng.poly_eval(groups, g2=g2)[0]}
                if not a.only_eval:
                    variants['b_composition_sample'] = composition
                got = variants['a_poly_eval']()          # correct and warm
                if not a.only_eval:
                    assert composition() == [got[k // m][k % m] for k in sample], (side, G, t, m, form)
                ts = {v: [] for v in variants}
                hosts, names = [], list(variants)
                before = smi()
                for r in range(a.reps):
                    for v in names[r % len(names):] + names[:r % len(names)]:
                        t0 = time.perf_counter()
                        variants[v]()
                        ts[v].append((time.perf_counter() - t0) * 1e3)
                        if v != 'a_poly_eval':
                            hosts.append(host['ms'])
                after = smi()
                row = {v: round(statistics.median(x), 3) for v, x in ts.items()}
                row['spread_min_max'] = {v: [round(min(x), 3), round(max(x), 3)] for v, x in ts.items()}
                if not a.only_eval:
                    scale = total / len(sample)
                    row['sample_identifiers'] = len(sample)
                    row['b_host_powers_sample'] = round(statistics.median(hosts), 3)
                    row['b_composition_scaled'] = round(row['b_composition_sample'] * scale, 1)
                    row['b_host_powers_scaled'] = round(row['b_host_powers_sample'] * scale, 1)
                    row['b_device_part_scaled'] = round(row['b_composition_scaled'] - row['b_host_powers_scaled'], 1)
                    row['poly_eval_over_composition'] = round(row['a_poly_eval'] / row['b_composition_scaled'], 5)
                row['sclk_power_before_after'] = [before, after]
                res['shapes']['%s_%dx(%d,%d)_%s' % (side, G, t, m, form)] = row
                print(side, G, t, m, form, row, file=sys.stderr, flush=True)
    res['config'] = eng.config_describe()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
