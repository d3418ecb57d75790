"""The facade's PointG1.verifyCellKzgProofBatch (and its *Async twin) on the GPU (tests/js/test_kzg_verify_cells.js): the cells of two blobs of 32 elements, four elements per
cell, against the test-only setup of kzg_cases.py; cells, proofs and [tau^c]G2 are Python's and the oracle's (kzg_verify_cells_cases.py)."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from kzg_cases import R, Setup
from kzg_cells_cases import monomial_setup
from kzg_verify_cells_cases import Call, random_blob, bumped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_kzg_verify_cells_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    setup = Setup(oracle, eng)
    rnd = random.Random(708)
    call = Call([random_blob(setup, 5, 2, rnd) for _ in range(2)])
    for b, k in [(0, 0), (1, 15), (0, 7), (1, 1), (0, 0)]:
        call.add(b, k)
    cases = {'monomial': [p.hex() for p in monomial_setup(setup, 5)], 'commitments': [c.hex() for c in call.commitments], 'commitment_index': call.ci, 'cell_index': call.ki,
             'cells': [c.hex() for c in call.cells], 'tampered': bumped(call.cells[2], 3).hex(), 'proofs': [p.hex() for p in call.proofs],
             'tau_c': setup.tau_g2(pow(setup.tau, 4, R)).hex(), 'tau': setup.tau_g2().hex(), 'seed': bytes(range(32)).hex()}
    del eng
    path = tmp_path / 'kzg_verify_cells_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_kzg_verify_cells.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS KZG verify cells ok' in out.stdout, out.stdout + out.stderr
