"""Times nbls_groth16_verify and nbls_groth16_prepare_inputs and writes profiles/groth16.json.  No time is a pass condition.
  shapes  n = 1 / 64 / 1024 / 8192 proofs, each at m = 1, 16 and 328 public inputs (the largest, 8192 x 328 = 2.7 M inputs, is inside the call's bound of 2^24: none is left out)
  cases   all valid, statuses asked for | one proof wrong, statuses asked for (the per-proof pass) | one proof wrong, no statuses (the fast reject) | prepare_inputs alone
  data    a test-only key with a known trapdoor; A_i, B_i from a pool of 64 (a, b) pairs, the inputs random, C_i = [c_i]G1 solved for them (get_public_keys)
Beside them the composition of the calls that existed before, interleaved call by call in the same run: three decoder calls (A, B, C), nbls_g1_msm_rows for the L_i (n rows
over IC_0 .. IC_m, the scalar of IC_0 = 1), and per proof ONE four-pair nbls_miller_product with the final exponentiation -- that last part ON A SAMPLE of proofs, scaled to n.
The library is called through ctypes on buffers packed once, so that the times are the calls' (the binding's packing of 2.7 M Python integers would take longer than the device).
Medians of `reps` calls after one warm-up call, min and max beside them; rocm-smi's shader clock and power are read right before and right after every shape.
--sums-shape NxM runs nbls_groth16_input_sums alone at that shape (for a kernel trace: 8192x16 and 8192x328); with --merge-trace CSV it adds that trace's kernel rows to the
JSON file, with the time it takes to read n * m * 32 bytes at the 6.3 TB/s that HBM delivers on this part.
usage: python tools/groth16_bench.py [--reps R] [--sample S] [--out FILE] [--n 1,64,1024,8192] [--m 1,16,328] [--sums-shape NxM [--merge-trace CSV]]"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from groth16_cases import R, Key, b32   # noqa: E402

HBM_TBS = 6.3


def smi():
    try:
        o = subprocess.run(['rocm-smi', '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20).stdout
        c = next(iter(json.loads(o).values()))
        sclk = [v for k, v in c.items() if 'sclk' in k.lower()]
        pw = [v for k, v in c.items() if 'power' in k.lower() and 'W' in k]
        return (sclk[0] if sclk else '?'), (pw[0] if pw else '?')
    except Exception as e:   # noqa: BLE001
        return '?', repr(e)[:40]


def interleaved(fs, reps):
    """{name: f} -> {name: median / min / max in ms}: one warm-up call each, then `reps` rounds that call every f once, in turn"""
    for f in fs.values():
        f()
    ts = {k: [] for k in fs}
    for _ in range(reps):
        for k, f in fs.items():
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for k, v in ts.items()}


def merge_trace(path, out, shape):
    n, m = shape
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get('Name') or r.get('KernelName') or ''
            if 'g16_' in name:
                rows[re.search(r'g16_\w+', name).group(0)] = {k: r[k] for k in r if k not in ('Name', 'KernelName')}
    res = json.load(open(out))
    res.setdefault('kernel_trace', {'what': 'rocprofv3 --kernel-trace --stats of `python tools/groth16_bench.py --sums-shape NxM`: eleven calls of nbls_groth16_input_sums a shape'})
    res['kernel_trace']['%dx%d' % shape] = {'kernels': rows, 'matrix_bytes': n * m * 32, 'hbm_read_us_at_%.1f_TBs' % HBM_TBS: round(n * m * 32 / (HBM_TBS * 1e12) * 1e6, 2)}
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'groth16.json'))
    ap.add_argument('--n', default='1,64,1024,8192')
    ap.add_argument('--m', default='1,16,328')
    ap.add_argument('--sums-shape', default=None)
    ap.add_argument('--merge-trace', default=None)
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.sums_shape.split('x')) if a.sums_shape else None
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out, shape)
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    lib, h = eng.lib, eng.h
    rnd = random.Random(2025)
    if shape:
        for n, m in [shape]:
            mat = b''.join(b32(rnd.randrange(R)) for _ in range(n * m))
            ws = b''.join(b32(rnd.randrange(1 << 63, 1 << 64)) for _ in range(n))
            out, st = C.create_string_buffer(32 * (m + 1)), C.create_string_buffer(n)
            t = interleaved({'input_sums': lambda: eng._chk(lib.nbls_groth16_input_sums(h, n, m, mat, ws, None, out, st))}, 10)
            print('input_sums (whole call, copies included)', n, m, t, file=sys.stderr, flush=True)
        return None
    import oracle_py
    oracle = oracle_py.load()
    ns, ms = [int(v) for v in a.n.split(',') if v], [int(v) for v in a.m.split(',') if v]
    res = {'reps': a.reps, 'sample': a.sample, 'shapes': {}, 'left_out': [], 'what': __doc__.split('usage:')[0].strip()}
    pool = 64
    for m in ms:
        key = Key(oracle, m, rnd)
        ic48 = eng.get_public_keys([b32(k) for k in key.ic])
        vk = eng.groth16_vk(key.g1(key.alpha), key.g2(key.beta), key.g2(key.gamma), key.g2(key.delta), ic48)
        ic_aff = eng.decompress_batch(b''.join(ic48))[0]
        ab = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(pool)]
        a48 = eng.get_public_keys([b32(x[0]) for x in ab])
        b96 = [key.g2(x[1]) for x in ab]
        fixed_g1 = key.g1_aff(key.alpha)
        fixed_g2 = [key.g2_aff(-key.gamma), key.g2_aff(-key.delta), key.g2_aff(-key.beta)]
        dinv = pow(key.delta, -1, R)
        for n in ns:
            if n * m > 1 << 24:
                res['left_out'].append([n, m])
                continue
            xs = [[rnd.randrange(R) for _ in range(m)] for _ in range(n)]
            cs = [(ab[i % pool][0] * ab[i % pool][1] - key.alpha * key.beta - key.gamma * key.l_scalar(x)) * dinv % R for i, x in enumerate(xs)]
            c48 = eng.get_public_keys([b32(c) for c in cs])
            proofs = b''.join(a48[i % pool] + b96[i % pool] + c48[i] for i in range(n))
            mat = b''.join(b32(v) for x in xs for v in x)
            wrong = n // 2
            bad = bytearray(mat)
            bad[32 * (wrong * m + m - 1):32 * (wrong * m + m)] = b32((xs[wrong][m - 1] + 1) % R)
            bad = bytes(bad)
            ok, st, out48 = C.c_int(0), C.create_string_buffer(n), C.create_string_buffer(48 * n)
            before = smi()

            def verify(inputs, status):
                eng._chk(lib.nbls_groth16_verify(h, vk.h, n, proofs, inputs, None, C.byref(ok), st if status else None))
                return ok.value
            assert verify(mat, True) == 1 and st.raw == bytes(n)
            assert verify(bad, True) == 0 and [i for i, v in enumerate(st.raw) if v] == [wrong] and st.raw[wrong] == 9
            assert verify(bad, False) == 0
            # the composition: the decoders and the rows over all n, the pairings on a sample
            s = min(n, a.sample)
            a_all, b_all, c_all = b''.join(a48[i % pool] for i in range(n)), b''.join(b96[i % pool] for i in range(n)), b''.join(c48)
            rows = b''.join(b32(1) + mat[32 * m * i:32 * m * (i + 1)] for i in range(n))
            aff = C.create_string_buffer(96 * n); aff2 = C.create_string_buffer(192 * n); l_out = C.create_string_buffer(96 * n); f12 = C.create_string_buffer(576)
            got = {}

            def decoders():
                eng._chk(lib.nbls_g1_decompress_batch(h, n, a_all, aff, st))
                got['a'] = aff.raw
                eng._chk(lib.nbls_g2_decompress_batch(h, n, b_all, aff2, st))
                got['b'] = aff2.raw
                eng._chk(lib.nbls_g1_decompress_batch(h, n, c_all, aff, st))
                got['c'] = aff.raw

            def l_rows():
                eng._chk(lib.nbls_g1_msm_rows(h, m + 1, ic_aff, n, rows, l_out, st))
                got['l'] = l_out.raw

            def pairings():
                for i in range(s):
                    g1s = got['a'][96 * i:96 * i + 96] + got['l'][96 * i:96 * i + 96] + got['c'][96 * i:96 * i + 96] + fixed_g1
                    g2s = got['b'][192 * i:192 * i + 192] + b''.join(fixed_g2)
                    eng._chk(lib.nbls_miller_product(h, 4, g1s, g2s, 1, 0, f12, st))
                    assert f12.raw[47] == 1 and not any(f12.raw[:47]) and not any(f12.raw[48:]), i
            row = interleaved({'verify_all_valid': lambda: verify(mat, True), 'verify_one_wrong_statuses': lambda: verify(bad, True), 'verify_one_wrong_fast_reject': lambda: verify(bad, False),
                               'prepare_inputs': lambda: eng._chk(lib.nbls_groth16_prepare_inputs(h, vk.h, n, mat, out48, st)),
                               'composition_decoders': decoders, 'composition_msm_rows': l_rows, 'composition_pairings_sample': pairings}, a.reps)
            row['composition_sample_proofs'] = s
            row['composition_scaled_ms'] = round(row['composition_decoders']['median_ms'] + row['composition_msm_rows']['median_ms'] + row['composition_pairings_sample']['median_ms'] * n / s, 3)
            row['verify_all_valid_vs_composition'] = round(row['composition_scaled_ms'] / row['verify_all_valid']['median_ms'], 2)
            row['proofs_per_s_all_valid'] = round(n / row['verify_all_valid']['median_ms'] * 1e3)
            row['sclk_power_before_after'] = [before, smi()]
            res['shapes']['%dx%d' % (n, m)] = row
            print(n, m, row, file=sys.stderr, flush=True)
        vk.close()
    res['config'] = eng.config_describe()
    print(json.dumps(res, sort_keys=True))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')
    return None


if __name__ == '__main__':
    main()
