"""Times nbls_kzg_verify_cells at the mainnet cell size (N = 4096, 64 elements per cell) and writes profiles/kzg_verify_cells.json.  No time is a pass condition.
  Cells and proofs of eight distinct random blobs come from the device's own prover against a test-only monomial basis (kzg_cases.TAU), the commitments from Python
  integers; larger calls repeat them under further commitment indices (the device does the same work for a repeated commitment or cell):
    128 cells of 1 blob | 1,024 cells = 8 cells of each of 128 commitments | 8,192 cells = 64 cells of each of 128 commitments
  Per shape, the raw call on packed arguments (the binding's joining of 16 MB of cells is no part of the subject), a host clock around the call, which ends in the read-back:
    accept        every cell valid: the combined check alone
    reject_fast   one element of one cell changed, status == NULL: the combined check alone
    reject        the same with statuses: the combined check, then the per-cell pass
  Medians of `reps` calls after one warm-up call (tables of roots and shifts, scratch slots, code objects), min and max beside them; rocm-smi's shader clock and power right
  before and after every shape.
--trace-workload: nothing is timed; `reps` times the accepting and the rejecting call on 8,192 cells and nbls_fr_ntt(log2_n = 6, to coefficients, 8,192 rows, shift h_k) --
the route the transform kernel offers for the same coefficients -- for a kernel trace taken around the process (the kernels' own times are that trace's).
usage: python tools/kzg_verify_cells_bench.py [--reps R] [--out FILE] [--trace-workload]"""
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
from kzg_cases import R, TAU, Setup, b32, blob_bytes, eval_roots   # noqa: E402
from kzg_cells_cases import cell_shift   # noqa: E402
from kzg_bench import smi, timed, g1   # noqa: E402

LOG2_N, LOG2_CELL = 12, 6
SHAPES = [(128, 1), (1024, 128), (8192, 128)]      # (cells, commitments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kzg_verify_cells.json'))
    ap.add_argument('--trace-workload', action='store_true')
    a = ap.parse_args()
    pkg = importlib.import_module('noble-bls12-381_amd')
    import oracle_py
    eng = pkg.Engine(0)
    rnd = random.Random(2027)
    N, per, c = 1 << LOG2_N, 2 << (LOG2_N - LOG2_CELL), 1 << LOG2_CELL
    distinct = [[rnd.randrange(R) for _ in range(N)] for _ in range(8)]
    t, powers = 1, []
    for _ in range(N):
        powers.append(t)
        t = t * TAU % R
    su = eng.kzg_monomial_setup(LOG2_N, g1(eng, powers))
    cells, proofs, st = eng.kzg_compute_cells_and_proofs(su, LOG2_CELL, [blob_bytes(f) for f in distinct])
    assert st == bytes(8)
    commitments = g1(eng, [eval_roots(f, TAU, LOG2_N) for f in distinct])
    tau_c = Setup(oracle_py.load(), eng).tau_g2(pow(TAU, c, R))
    seed = bytes(range(32))

    def packed(n, nc):
        """cell j of the call: cell (j // nc) % 128 of commitment j % nc, which is blob (j % nc) % 8"""
        ci = [j % nc for j in range(n)]
        ki = [(j // nc) % per for j in range(n)]
        arr = C.c_uint32 * n
        return [nc, b''.join(commitments[i % 8] for i in range(nc)), n, arr(*ci), arr(*ki), b''.join(cells[ci[j] % 8][ki[j]] for j in range(n)),
                b''.join(proofs[ci[j] % 8][ki[j]] for j in range(n))]

    def call(args, per_item, want_ok):
        ok, stat = C.c_int(-1), C.create_string_buffer(args[2])
        r = eng.lib.nbls_kzg_verify_cells(eng.h, su.h, LOG2_CELL, *args, tau_c, seed, C.byref(ok), stat if per_item else None)
        assert r == 0 and ok.value == want_ok, (r, ok.value)
        return stat.raw

    def tampered(args):
        bad = list(args)
        j = args[2] // 2
        at = 32 * c * j + 32 * 5 + 31
        bad[5] = args[5][:at] + bytes([args[5][at] ^ 1]) + args[5][at + 1:]
        return bad, j

    if a.trace_workload:
        good = packed(8192, 128)
        bad, _ = tampered(good)
        shifts = b''.join(b32(cell_shift(k, LOG2_N, LOG2_CELL)) for k in good[4])
        out = C.create_string_buffer(len(good[5]))
        for _ in range(a.reps):
            call(good, True, 1)
            call(bad, True, 0)
            assert eng.lib.nbls_fr_ntt(eng.h, LOG2_CELL, 0, 8192, good[5], shifts, out, None) == 0
        return
    res = {'reps': a.reps, 'log2_n': LOG2_N, 'log2_cell': LOG2_CELL, 'shapes': {}, 'what': __doc__.split('usage:')[0].strip()}
    for n, nc in SHAPES:
        good = packed(n, nc)
        bad, j = tampered(good)
        before = smi()
        assert call(good, True, 1) == bytes(n)
        assert call(bad, True, 0) == bytes(9 if i == j else 0 for i in range(n))
        row = {'commitments': nc, 'accept': timed(lambda: call(good, True, 1), a.reps), 'reject_fast': timed(lambda: call(bad, False, 0), a.reps),
               'reject': timed(lambda: call(bad, True, 0), a.reps)}
        row['sclk_power_before_after'] = [before, smi()]
        res['shapes'][str(n)] = row
        print('cells', n, row, file=sys.stderr, flush=True)
    res['config'] = eng.config_describe()
    print(json.dumps(res, sort_keys=True))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
