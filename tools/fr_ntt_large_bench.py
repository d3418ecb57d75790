"""Times nbls_fr_ntt_large and nbls_fr_ntt_dev and writes profiles/fr_ntt_large.json.  No time is a pass condition.
  shapes  2^13 / 2^16 / 2^20 / 2^24 elements with one polynomial, 2^16 with 256; both directions; random canonical elements, one shift per polynomial
  routes  the host-buffer call (wall clock: copies included) | the device-resident call on torch buffers, in place (HIP events on the call's stream) | the composition of
          the calls that existed before: a numpy transpose, nbls_fr_ntt over the 2^t columns of 2^K elements, a transpose back, nbls_fr_ntt over the 2^K rows of 2^t elements
          with the shifts omega_N^rev_K(B) made from Python integers.  The composition is timed WITHOUT a caller's shift (it would need a third pass over the
          elements), the new calls WITH one
  The three are interleaved call by call in one run, medians of `reps` calls after one warm-up call each, and their bytes are compared before anything is timed.
  sweeps  the device-resident call at 2^20 and 2^24 for every NBLS_TUNE_NTT_PASS_BITS 1 .. 9, and at 2^20 and 2^23 for NBLS_TUNE_NTT_TAIL_BITS 11 against 12 (2^24 leaves
          thirteen global stages at t = 11: refused)
  sparse  at 2^24: four coefficients, shift 7, 256 sampled positions against the closed form, then the way back against the input's SHA-256
  copy    a device-to-device copy of the 2^24-element buffer, timed the same way: bytes read + written per second; beside every launch of the trace the time that
          64 bytes per element (one read, one write) take at that rate -- a figure to read the launch against, not a target
  trace   one run of this file under `rocprofv3 --kernel-trace --stats` (--trace-run: six calls a direction at 2^24 and nothing else; no counters), folded into per-launch
          medians
usage: python tools/fr_ntt_large_bench.py [--reps R] [--out FILE] [--no-trace] [--max-log2 L]"""
import argparse
import csv
import ctypes as C
import glob
import hashlib
import importlib
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np   # noqa: E402
from kzg_cases import R   # noqa: E402
from kzg_cells_cases import rows   # noqa: E402
from fr_ntt_large_cases import block_shift, sparse_eval, split_runs   # noqa: E402

TAIL, PASS_DEFAULT = 12, 8
SHAPES = [(13, 1), (16, 1), (16, 256), (20, 1), (24, 1)]


def random_rows(log2_n, n, seed):
    a = np.random.default_rng(seed).integers(0, 256, size=(n << log2_n, 32), dtype=np.uint8)
    a[:, 0] &= 0x3f
    return a.tobytes()


def med(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}


class Routes:
    def __init__(self, eng, torch):
        self.eng, self.lib, self.h, self.torch = eng, eng.lib, eng.h, torch

    def host(self, log2_n, d, raw, sh, out):
        self.eng._chk(self.lib.nbls_fr_ntt_large(self.h, log2_n, d, len(raw) // (32 << log2_n), raw, sh, out, None))

    def dev_ms(self, log2_n, d, n, buf, src, sh):
        """one in-place call on `buf` (refilled from `src` first), between two events on the current stream -> ms"""
        t = self.torch
        buf.copy_(src)
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        s = t.cuda.current_stream()
        a.record(s)
        self.eng.fr_ntt_dev(log2_n, n, buf.data_ptr(), bool(d), buf.data_ptr(), None if sh is None else sh.data_ptr(), None, stream=s.cuda_stream)
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b)

    def composition(self, log2_n, d, raw, n):
        """the calls that existed before, per polynomial: fact 2 and fact 3 of the header's note on nbls_fr_ntt_large"""
        k, t = log2_n - TAIL, TAIL
        sb = rows([block_shift(log2_n, t, b) for b in range(1 << k)])

        def ntt(bits, count, data, shifts):
            o = C.create_string_buffer(len(data))
            self.eng._chk(self.lib.nbls_fr_ntt(self.h, bits, d, count, data, shifts, o, None))
            return np.frombuffer(o, dtype=np.uint8)

        def columns(a):          # every column of every polynomial through the transform of size 2^k, one call
            cols = np.ascontiguousarray(a.reshape(n, 1 << k, 1 << t, 32).transpose(0, 2, 1, 3)).tobytes()
            return np.ascontiguousarray(ntt(k, n << t, cols, None).reshape(n, 1 << t, 1 << k, 32).transpose(0, 2, 1, 3)).reshape(-1)

        def tails(a):
            return ntt(t, n << k, a.tobytes(), sb * n)
        a = np.frombuffer(raw, dtype=np.uint8)
        return (tails(columns(a)) if d else columns(tails(a))).tobytes()


def sparse_check(eng, log2_n):
    n, shift = 1 << log2_n, 7
    terms = [(0, 5), (4095 * (1 << (log2_n - 12)) + 1, R - 3), (1 << (log2_n - 1), 0x1234567890abcdef), (n - 1, R - 1)]
    coef = bytearray(32 * n)
    for e, c in terms:
        coef[32 * e:32 * e + 32] = c.to_bytes(32, 'big')
    coef, sh = bytes(coef), rows([shift])
    rnd = random.Random(2400)
    at = {0, n - 1, 4095, 4096} | {(1 << b) - 1 for b in range(1, log2_n + 1)} | {1 << b for b in range(log2_n)}
    while len(at) < 256:
        at.add(rnd.randrange(n))
    vals, st = eng.fr_ntt_large(log2_n, coef, True, sh)
    bad = [j for j in sorted(at) if vals[32 * j:32 * j + 32] != sparse_eval(terms, log2_n, j, shift).to_bytes(32, 'big')]
    back, st2 = eng.fr_ntt_large(log2_n, vals, False, sh)
    ok = not bad and st == [0] and st2 == [0] and hashlib.sha256(back).digest() == hashlib.sha256(coef).digest()
    assert ok, ('sparse check at 2^%d' % log2_n, bad[:4], st, st2)
    return {'log2_n': log2_n, 'positions': len(at), 'mismatches': len(bad), 'round_trip_sha256_equal': True}


def trace_run(eng, torch, log2_n, calls):
    """what the profiler watches: one warm-up call a direction, then `calls` towards the values, then `calls` back, in place on one buffer"""
    n = 1
    buf = torch.frombuffer(bytearray(random_rows(log2_n, n, 24)), dtype=torch.uint8).cuda()
    sh = torch.frombuffer(bytearray(rows([7])), dtype=torch.uint8).cuda()
    for d in (True, False):
        eng.fr_ntt_dev(log2_n, n, buf.data_ptr(), d, buf.data_ptr(), sh.data_ptr(), None)
    for d in (True, False):
        for _ in range(calls):
            eng.fr_ntt_dev(log2_n, n, buf.data_ptr(), d, buf.data_ptr(), sh.data_ptr(), None)
    torch.cuda.synchronize()


def fold_trace(directory, log2_n, calls, copy_bytes_per_s):
    files = glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        return {'error': 'no kernel_trace.csv under the profiler output'}
    disp = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            name = r.get('Kernel_Name') or r.get('Name') or ''
            if 'kzg_ntt_pass_kernel' in name or 'kzg_ntt_tail_kernel' in name:
                disp.append((int(r['Start_Timestamp']), 'pass' if 'pass' in name else 'tail', (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6))
    disp.sort()
    runs = split_runs(log2_n - TAIL, PASS_DEFAULT)
    per = len(runs) + 1
    if len(disp) != per * (2 + 2 * calls):
        return {'error': 'expected %d launches of the two kernels, saw %d' % (per * (2 + 2 * calls), len(disp))}
    floor = round(64 * (1 << log2_n) / copy_bytes_per_s * 1e3, 4)
    out = {'what': 'rocprofv3 --kernel-trace --stats of `python tools/fr_ntt_large_bench.py --trace-run`: medians over %d calls a direction at 2^%d, one polynomial, shift 7, '
                   'in launch order; floor_ms = 64 bytes per element at the copy rate this run measured' % (calls, log2_n), 'floor_ms_64B_per_element': floor}
    for di, dname in enumerate(('to_evals', 'to_coeffs')):
        base = per * 2 + di * per * calls
        names = ['stages %d..%d' % (j0, j1 - 1) for j0, j1 in runs] + ['tails']
        if dname == 'to_coeffs':
            names = names[::-1]
        launches = []
        for pos in range(per):
            v = [disp[base + c * per + pos] for c in range(calls)]
            assert len({x[1] for x in v}) == 1
            launches.append({'launch': names[pos], 'kernel': 'kzg_ntt_%s_kernel' % v[0][1], **med([x[2] for x in v])})
        out[dname] = {'launches': launches, 'sum_of_medians_ms': round(sum(x['median_ms'] for x in launches), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fr_ntt_large.json'))
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--max-log2', type=int, default=24)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module('noble-bls12-381_amd')
    eng = pkg.Engine(0)
    if a.trace_run:
        return trace_run(eng, torch, min(24, a.max_log2), 6)
    rt = Routes(eng, torch)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    res = {'reps': a.reps, 'what': __doc__.split('usage:')[0].strip(), 'default_plan': {'tail_bits': TAIL, 'pass_bits': PASS_DEFAULT}, 'shapes': {}, 'sweep_pass_bits': {}, 'sweep_tail_bits': {}}
    top = min(24, a.max_log2)
    # the copy rate
    big = torch.empty(32 << top, dtype=torch.uint8, device='cuda')
    src = torch.zeros(32 << top, dtype=torch.uint8, device='cuda')
    ts = []
    for i in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); big.copy_(src); e1.record(); e1.synchronize()
        if i:
            ts.append(e0.elapsed_time(e1))
    copy_rate = 2 * (32 << top) / (statistics.median(ts) * 1e-3)
    res['copy'] = {'bytes': 32 << top, **med(ts), 'read_plus_write_TB_per_s': round(copy_rate / 1e12, 3)}
    del big, src
    for log2_n, n in SHAPES:
        if log2_n > top:
            continue
        raw = random_rows(log2_n, n, 1000 + log2_n + n)
        shifts = rows([random.Random(log2_n + i).randrange(1, R) for i in range(n)])
        d_src, d_buf, d_sh = dev(raw), dev(raw), dev(shifts)
        out = C.create_string_buffer(len(raw))
        row = {'runs_of_global_stages': split_runs(log2_n - TAIL, PASS_DEFAULT)}
        for d, dname in ((1, 'to_evals'), (0, 'to_coeffs')):
            # the bytes first: host call == device call (with the shifts), host call == composition (without)
            rt.host(log2_n, d, raw, shifts, out)
            rt.dev_ms(log2_n, d, n, d_buf, d_src, d_sh)
            assert d_buf.cpu().numpy().tobytes() == out.raw, (log2_n, n, dname, 'device-resident call')
            rt.host(log2_n, d, raw, None, out)
            assert rt.composition(log2_n, d, raw, n) == out.raw, (log2_n, n, dname, 'composition')
            t = {'host_call': [], 'device_call': [], 'composition': []}
            for i in range(a.reps + 1):
                t0 = time.perf_counter(); rt.host(log2_n, d, raw, shifts, out); t1 = time.perf_counter()
                dm = rt.dev_ms(log2_n, d, n, d_buf, d_src, d_sh)
                t2 = time.perf_counter(); rt.composition(log2_n, d, raw, n); t3 = time.perf_counter()
                if i:
                    t['host_call'].append((t1 - t0) * 1e3); t['device_call'].append(dm); t['composition'].append((t3 - t2) * 1e3)
            row[dname] = {k: med(v) for k, v in t.items()}
            row[dname]['composition_over_host_call'] = round(row[dname]['composition']['median_ms'] / row[dname]['host_call']['median_ms'], 2)
            row[dname]['device_call_floor_ms_64B_per_element_per_launch'] = round(64 * (n << log2_n) / copy_rate * 1e3 * (len(row['runs_of_global_stages']) + 1), 4)
        res['shapes']['2^%d x %d' % (log2_n, n)] = row
        print(log2_n, n, row, file=sys.stderr, flush=True)
        del d_src, d_buf, d_sh

    def sweep(key, log2_n, name, values):
        raw = random_rows(log2_n, 1, 2000 + log2_n)
        d_src, d_buf, d_sh = dev(raw), dev(raw), dev(rows([7]))
        try:
            for v in values:
                eng.set_ntt_plan(**{name: v})
                entry = {}
                if name == 'pass_bits':
                    entry['runs'] = split_runs(log2_n - TAIL, v)
                for d, dname in ((1, 'to_evals'), (0, 'to_coeffs')):
                    ts = [rt.dev_ms(log2_n, d, 1, d_buf, d_src, d_sh) for _ in range(a.reps + 1)][1:]
                    entry[dname] = med(ts)
                res[key].setdefault('2^%d' % log2_n, {})[str(v)] = entry
                print(key, log2_n, v, entry, file=sys.stderr, flush=True)
        finally:
            eng.set_ntt_plan(0, 0)
    for log2_n in (20, 24):
        if log2_n <= top:
            sweep('sweep_pass_bits', log2_n, 'pass_bits', range(1, 10))
    for log2_n in (20, 23):
        if log2_n <= top:
            sweep('sweep_tail_bits', log2_n, 'tail_bits', (11, 12))
    res['sparse_check'] = sparse_check(eng, top)
    if not a.no_trace:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__), '--trace-run', '--max-log2', str(top)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                res['kernel_trace'] = fold_trace(tmp, top, 6, copy_rate) if p.returncode == 0 else {'error': 'rocprofv3 exit %d: %s' % (p.returncode, p.stderr[-300:])}
                stats = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
                if stats and a.out:          # the profiler's own per-kernel table beside the JSON file
                    shutil.copyfile(stats[0], os.path.splitext(a.out)[0] + '_kernel_stats.csv')
            except (OSError, subprocess.TimeoutExpired) as e:
                res['kernel_trace'] = {'error': repr(e)[:200]}
    res['config'] = eng.config_describe()
    print(json.dumps(res, sort_keys=True))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')
    return None


if __name__ == '__main__':
    main()
