"""The facade's PointG1.KzgSetup and PointG1.blobToKzgCommitments / computeKzgProofs / computeBlobKzgProofs (and *Async) on the GPU (tests/js/test_kzg_prove.js): three blobs of 64
elements against the test-only setup of kzg_cases.py; every expected byte is the oracle's (kzg_prove_cases.py)."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from kzg_cases import R, Setup, roots
from kzg_prove_cases import lagrange_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_kzg_prover_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    setup = Setup(oracle, eng)
    rnd = random.Random(606)
    fs = [[rnd.randrange(R) for _ in range(64)], [rnd.randrange(1, R)] * 64, [rnd.randrange(R) for _ in range(64)]]
    zs = [rnd.randrange(R), rnd.randrange(R), roots(6)[63]]
    opened = [setup.proof(f, z, 6) for f, z in zip(fs, zs)]
    blobs = [setup.blob_case(f, 6) for f in fs]
    lag = lagrange_setup(setup, 6)
    cases = {'lagrange': [p.hex() for p in lag], 'blobs': [b[0].hex() for b in blobs], 'commitments': [b[1].hex() for b in blobs], 'blob_proofs': [b[2].hex() for b in blobs],
             'zs': ['%064x' % z for z in zs], 'ys': ['%064x' % y for y, _ in opened], 'proofs': [p.hex() for _, p in opened], 'r': '%064x' % R}
    del eng
    path = tmp_path / 'kzg_prove_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_kzg_prove.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS KZG prover ok' in out.stdout, out.stdout + out.stderr
