"""Times nbls_groth16_prove and writes profiles/groth16_prove.json.  No time is a pass condition.
  shapes  N = 2^12 / 2^16 / 2^20 constraints, n_vars = N, 1 public input: three entries a row of A (one a row of B and of C), plus one row of A with N / 2 entries; 1 and 8
          witnesses a call
  data    a satisfied instance (row j: (z_j + 2 z_(j+1) + 3 z_(j+7)) * z_(j+3) = (a_j b_j) * z_0; the last row's A sums the first N / 2 variables); the key's points are subgroup points from a
          pool of 1024 in G1 and 128 in G2, tiled -- NOT a key of any trapdoor: the proofs are compared with the composition's, not verified (tests/test_gpu_groth16_prove.py
          verifies proofs against real keys)
Beside it the composition of the calls that existed before, for ONE witness, interleaved call by call in the same run: the matrix products in Python integers ON A SAMPLE of
rows, scaled to N (the long row in full); nbls_fr_ntt_large three rows to coefficients, three rows to the values on the coset of 7, the pointwise step in Python integers ON A
SAMPLE of elements, scaled, one row back; nbls_g1_msm / nbls_g2_msm from host points for A, B1, B and the l / h part of C; the final additions [1]C' + [s]A + [r]B1 - [r s]delta
through nbls_g1_msm.  Its three points, compressed, must equal the call's proof.
Medians of `reps` calls after one warm-up call, min and max beside them.  --trace-run LOG2 makes one key and three calls of one witness at that size and nothing else (for
rocprofv3 --kernel-trace --stats); --merge-trace CSV adds that trace's kernel rows to the JSON file.
usage: python tools/groth16_prove_bench.py [--reps R] [--sample S] [--out FILE] [--log2 12,16,20] [--trace-run LOG2 | --merge-trace CSV]"""
import argparse
import csv
import ctypes as C
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
from kzg_cases import R, b32, bitrev   # noqa: E402

G2_GEN = bytes.fromhex('024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8'
                       '13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e'
                       '0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801'
                       '0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be')


def interleaved(fs, reps):
    """{name: f} -> {name: median / min / max in ms}: one warm-up call each, then `reps` rounds that call every f once, in turn"""
    for f in fs.values():
        f()
    ts = {k: [] for k in fs}
    for _ in range(reps):
        for k, f in fs.items():
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for k, v in ts.items()}


def tile(pool, width, count):
    reps = -(-count // (len(pool) // width))
    return (pool * reps)[:count * width]


class Shape:
    """the instance, its witness and the key's points at N = 2^log2_n"""

    def __init__(self, eng, pkg, log2_n, rnd, g1c, g1a, g2c, g2a):
        N = self.N = 1 << log2_n
        self.log2_n, self.nv, self.m = log2_n, N, 1
        z = self.z = [1] + [rnd.getrandbits(254) for _ in range(N - 1)]
        self.a = [(z[j] + 2 * z[(j + 1) % N] + 3 * z[(j + 7) % N]) % R for j in range(N - 1)] + [sum(z[:N // 2]) % R]
        self.b = [z[(j + 3) % N] for j in range(N)]
        self.c = [x * y % R for x, y in zip(self.a, self.b)]
        u32 = lambda v: (C.c_uint32 * len(v))(*v)
        a_cols = [c for j in range(N - 1) for c in (j, (j + 1) % N, (j + 7) % N)] + list(range(N // 2))
        a_vals = (b32(1) + b32(2) + b32(3)) * (N - 1) + b32(1) * (N // 2)
        a_offs = [3 * j for j in range(N)] + [3 * (N - 1) + N // 2]
        ones = list(range(N + 1))
        self.keep = [u32(a_offs), u32(a_cols), a_vals, u32(ones), u32([(j + 3) % N for j in range(N)]), b32(1) * N, u32(ones), u32([0] * N), b''.join(b32(v) for v in self.c)]
        na = N - 2
        self.pts = [g1c[:48], g1c[48:96], g2c[:96], g1c[96:144], g2c[96:192], tile(g1c, 48, N), tile(g1c[48:], 48, N), tile(g2c, 96, N), tile(g1c[96:], 48, na), tile(g1c[144:], 48, N - 1)]
        # the same points affine, as the arrays the composition's sums read
        self.aff = {'a': tile(g1a, 96, N) + g1a[:96] + g1a[192:288], 'b1': tile(g1a[96:], 96, N) + g1a[96:192] + g1a[192:288], 'b2': tile(g2a, 192, N) + g2a[:192] + g2a[192:384],
                    'c': tile(g1a[192:], 96, na) + tile(g1a[288:], 96, N - 1), 'delta': g1a[192:288]}
        d = pkg.Groth16PkDesc(log2_n=log2_n, n_vars=N, n_public=1, n_constraints=N)
        as_ptr = lambda b: C.cast(b if not isinstance(b, bytes) else C.c_char_p(b), C.c_void_p)
        for f, b in zip([m + s for m in 'abc' for s in ('_rows', '_cols', '_vals32')], self.keep):
            setattr(d, f, as_ptr(b))
        for f, b in zip(('alpha_g1_48', 'beta_g1_48', 'beta_g2_96', 'delta_g1_48', 'delta_g2_96', 'a_query48', 'b_g1_query48', 'b_g2_query96', 'l_query48', 'h_query48'), self.pts):
            setattr(d, f, as_ptr(b))
        h = C.c_void_p()
        t0 = time.perf_counter()
        eng._chk(eng.lib.nbls_groth16_pk_create(eng.h, C.byref(d), None, C.byref(h)))
        self.pk_create_ms = round((time.perf_counter() - t0) * 1e3, 1)
        self.pk = pkg.Groth16Pk(eng.lib, h)
        self.zraw = b''.join(b32(v) for v in z)


def bench_shape(eng, sh, reps, sample, rnd):
    lib, h, N, L = eng.lib, eng.h, sh.N, sh.log2_n
    r, s = rnd.randrange(R), rnd.randrange(R)
    rs = b32(r) + b32(s)
    out1, st1 = C.create_string_buffer(192), C.create_string_buffer(1)
    out8, st8 = C.create_string_buffer(192 * 8), C.create_string_buffer(8)

    def prove1():
        eng._chk(lib.nbls_groth16_prove(h, sh.pk.h, 1, sh.zraw, rs, out1, st1))

    def prove8():
        eng._chk(lib.nbls_groth16_prove(h, sh.pk.h, 8, sh.zraw * 8, rs * 8, out8, st8))
    prove1()
    assert st1.raw == b'\0', st1.raw
    got = {}
    rows = sorted(rnd.sample(range(N - 1), min(sample, N - 1)))
    elems = sorted(rnd.sample(range(N), min(sample, N)))
    z = sh.z

    def matvec_sample():
        for j in rows:
            (z[j] + 2 * z[(j + 1) % N] + 3 * z[(j + 7) % N]) % R * z[(j + 3) % N] % R
        sum(z[:N // 2]) % R
    vec = [0] * (3 * N)
    for j in range(N):
        p = bitrev(j, L)
        vec[p], vec[N + p], vec[2 * N + p] = sh.a[j], sh.b[j], sh.c[j]
    v3 = b''.join(b32(v) for v in vec)
    sev3 = b32(7) * 3
    buf3, bufh, stn = C.create_string_buffer(96 * N), C.create_string_buffer(32 * N), C.create_string_buffer(3)
    kinv = pow(pow(7, N, R) - 1, -1, R)

    def transforms():
        eng._chk(lib.nbls_fr_ntt_large(h, L, 0, 3, v3, None, buf3, stn))
        eng._chk(lib.nbls_fr_ntt_large(h, L, 1, 3, buf3, sev3, buf3, stn))   # (the call stages its input before it writes its output)

    ev = memoryview(buf3).cast('B')   # (the values where the transforms leave them: no copy inside a timing)

    def pointwise_sample():
        for i in elems:
            x, y, w = (int.from_bytes(ev[32 * (k * N + i):32 * (k * N + i) + 32], 'big') for k in range(3))
            b32((x * y - w) * kinv % R)

    def pointwise_full_once():   # (outside the timing: the composition's h, for the comparison of the bytes)
        return b''.join(b32((int.from_bytes(ev[32 * i:32 * i + 32], 'big') * int.from_bytes(ev[32 * (N + i):32 * (N + i) + 32], 'big')
                             - int.from_bytes(ev[32 * (2 * N + i):32 * (2 * N + i) + 32], 'big')) * kinv % R) for i in range(N))
    transforms()
    hq = pointwise_full_once()

    def back():
        eng._chk(lib.nbls_fr_ntt_large(h, L, 0, 1, hq, sev3, bufh, stn))
    back()
    sa, sb = sh.zraw + b32(1) + b32(r), sh.zraw + b32(1) + b32(s)
    sc = sh.zraw[64:] + bufh.raw[:32 * (N - 1)]
    p96, p192, one = C.create_string_buffer(96), C.create_string_buffer(192), C.create_string_buffer(1)

    def msm(g2, n, pts, ks, key):
        o = p192 if g2 else p96
        eng._chk((lib.nbls_g2_msm if g2 else lib.nbls_g1_msm)(h, n, pts, ks, o, one))
        got[key] = o.raw

    def msms():
        msm(False, N + 2, sh.aff['a'], sa, 'A'); msm(False, N + 2, sh.aff['b1'], sb, 'B1'); msm(True, N + 2, sh.aff['b2'], sb, 'B'); msm(False, 2 * N - 3, sh.aff['c'], sc, 'C1')

    def final_sum():
        msm(False, 4, got['C1'] + got['A'] + got['B1'] + sh.aff['delta'], b32(1) + b32(s) + b32(r) + b32(-r * s % R), 'C')
    msms(); final_sum()
    ours = eng.compress_batch(got['A']) + eng.compress_batch(got['B'], g2=True) + eng.compress_batch(got['C'])
    assert ours == out1.raw, 'the composition and nbls_groth16_prove disagree'
    row = interleaved({'prove_1': prove1, 'prove_8': prove8, 'composition_matvec_sample': matvec_sample, 'composition_transforms': transforms,
                       'composition_pointwise_sample': pointwise_sample, 'composition_transform_back': back, 'composition_msms': msms, 'composition_final_sum': final_sum}, reps)
    assert out8.raw == out1.raw * 8 and st8.raw == bytes(8)
    med = lambda k: row[k]['median_ms']
    row['composition_scaled_ms'] = round(med('composition_matvec_sample') * (N - 1) / len(rows) + med('composition_transforms') + med('composition_pointwise_sample') * N / len(elems) +
                                         med('composition_transform_back') + med('composition_msms') + med('composition_final_sum'), 3)
    row['composition_device_calls_ms'] = round(med('composition_transforms') + med('composition_transform_back') + med('composition_msms') + med('composition_final_sum'), 3)
    row['prove_1_vs_composition'] = round(row['composition_scaled_ms'] / med('prove_1'), 2)
    row['prove_1_vs_composition_device_calls'] = round(row['composition_device_calls_ms'] / med('prove_1'), 2)
    row['prove_8_ms_per_proof'] = round(med('prove_8') / 8, 3)
    row['pk_create_ms'] = sh.pk_create_ms
    row['sample'] = len(rows)
    return row


def merge_trace(path, out):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get('Name') or r.get('KernelName') or ''
            rows[name[:120]] = {k: r[k] for k in r if k not in ('Name', 'KernelName')}
    res = json.load(open(out)) if os.path.exists(out) else {}
    res['kernel_trace'] = {'what': 'rocprofv3 --kernel-trace --stats of `python tools/groth16_prove_bench.py --trace-run LOG2`: the key creation and three calls of one witness', 'kernels': rows}
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'groth16_prove.json'))
    ap.add_argument('--log2', default='12,16,20')
    ap.add_argument('--trace-run', type=int, default=0)
    ap.add_argument('--merge-trace', default=None)
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    rnd = random.Random(2026)
    g1a, st = eng.point_mul_batch([b32(rnd.randrange(1, R)) for _ in range(1024)])
    g2a, st2 = eng.point_mul_batch([b32(rnd.randrange(1, R)) for _ in range(128)], pts=G2_GEN * 128, g2=True)
    assert not any(st) and not any(st2)
    g1c, g2c = eng.compress_batch(g1a), eng.compress_batch(g2a, g2=True)
    if a.trace_run:
        sh = Shape(eng, pkg, a.trace_run, rnd, g1c, g1a, g2c, g2a)
        out, st1 = C.create_string_buffer(192), C.create_string_buffer(1)
        for _ in range(3):
            eng._chk(eng.lib.nbls_groth16_prove(eng.h, sh.pk.h, 1, sh.zraw, b32(5) + b32(6), out, st1))
        assert st1.raw == b'\0'
        return None
    res = {'reps': a.reps, 'shapes': {}, 'what': __doc__.split('usage:')[0].strip()}
    for log2_n in [int(v) for v in a.log2.split(',') if v]:
        sh = Shape(eng, pkg, log2_n, rnd, g1c, g1a, g2c, g2a)
        row = bench_shape(eng, sh, a.reps, a.sample, rnd)
        res['shapes']['2^%d' % log2_n] = row
        print(log2_n, row, file=sys.stderr, flush=True)
        sh.pk.close()
        if a.out:   # (after every shape: a run cut short keeps what it measured)
            res['config'] = eng.config_describe()
            with open(a.out, 'w') as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write('\n')
    print(json.dumps(res, sort_keys=True))
    return None


if __name__ == '__main__':
    main()
