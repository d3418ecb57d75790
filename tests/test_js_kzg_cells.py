"""The facade's PointG1.frNtt / computeCells / KzgMonomialSetup / computeCellsAndKzgProofs (and *Async) on the GPU (tests/js/test_kzg_cells.js): two polynomials and three blobs of
32 elements against the test-only setup of kzg_cases.py; every expected byte is Python's or the oracle's (kzg_cells_cases.py)."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from kzg_cases import R, ZERO48, Setup, b32, blob_bytes
from kzg_cells_cases import to_evals, to_coeffs, cells, cell_proof, monomial_setup, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_kzg_cells_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    setup = Setup(oracle, eng)
    rnd = random.Random(707)
    vals = [[rnd.randrange(R) for _ in range(32)] for _ in range(2)]
    shifts = [rnd.randrange(1, R), R - 1]
    fs = [[rnd.randrange(R) for _ in range(32)], [rnd.randrange(R) for _ in range(32)], to_evals([rnd.randrange(1, R) for _ in range(4)] + [0] * 28, 5)]
    blobs = [blob_bytes(f) for f in fs]
    blobs[1] = blobs[1][:32 * 7] + b32(R) + blobs[1][32 * 8:]
    want_cells = [[rows(c).hex() for c in cells(f, 5, 2)] for f in fs]
    want_cells[1] = [bytes(128).hex()] * 16
    want_proofs = [[cell_proof(setup, to_coeffs(f, 5), k, 5, 2).hex() for k in range(16)] for f in fs]
    want_proofs[1] = [bytes(48).hex()] * 16
    assert want_proofs[2] == [ZERO48.hex()] * 16
    cases = {'values': [rows(v).hex() for v in vals], 'shifts': ['%064x' % s for s in shifts], 'coefficients': [rows(to_coeffs(v, 5, s)).hex() for v, s in zip(vals, shifts)],
             'plain_coefficients': [rows(to_coeffs(v, 5)).hex() for v in vals], 'blobs': [b.hex() for b in blobs], 'cells': want_cells, 'proofs': want_proofs,
             'monomial': [p.hex() for p in monomial_setup(setup, 5)], 'r': '%064x' % R}
    del eng
    path = tmp_path / 'kzg_cells_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_kzg_cells.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS KZG cells ok' in out.stdout, out.stdout + out.stderr
