"""The facade's PointG1.recoverCells / recoverCellsAndKzgProofs (and *Async) on the GPU (tests/js/test_kzg_recover.js): two blobs of 32 elements in 16 cells against the test-only
setup of kzg_cases.py; every expected byte is Python's or the oracle's (kzg_cells_cases.py), and the refused inputs are refused by kzg_recover_cases.py as well."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from kzg_cases import R, Setup, blob_bytes
from kzg_cells_cases import to_evals, cells, cell_proof, monomial_setup, rows
from kzg_recover_cases import BAD_CELLS, INCONSISTENT, recover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_kzg_recover_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    setup = Setup(oracle, eng)
    rnd = random.Random(717)
    coefs = [[rnd.randrange(R) for _ in range(32)] for _ in range(2)]
    fs = [to_evals(co, 5) for co in coefs]
    cs = [cells(f, 5, 2) for f in fs]
    indices = [rnd.sample(range(16), 8), rnd.sample(range(16), 9)]
    short = rnd.sample(range(16), 7)
    changed = list(cs[1][indices[1][0]])
    changed[3] = (changed[3] + 1) % R
    assert recover(short, [cs[0][k] for k in short], 5, 2)[0] == BAD_CELLS
    assert recover(indices[1], [changed] + [cs[1][k] for k in indices[1][1:]], 5, 2)[0] == INCONSISTENT
    cases = {'blobs': [blob_bytes(f).hex() for f in fs], 'cells': [[rows(c).hex() for c in blob] for blob in cs],
             'proofs': [[cell_proof(setup, co, k, 5, 2).hex() for k in range(16)] for co in coefs], 'indices': indices, 'short': short, 'changed': rows(changed).hex(),
             'monomial': [p.hex() for p in monomial_setup(setup, 5)]}
    del eng
    path = tmp_path / 'kzg_recover_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_kzg_recover.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS KZG recover ok' in out.stdout, out.stdout + out.stderr
