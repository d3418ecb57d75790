"""The facade's PointG1.verifyKzgProofBatch / verifyBlobKzgProofBatch (and *Async) on the GPU (tests/js/test_kzg.js): nine valid tuples and the tampered one from the test-only
setup of kzg_cases.py, blobs with hashlib challenges; hex, bytes and points in."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from kzg_cases import R, Setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_kzg_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    setup = Setup(oracle, eng)
    rnd = random.Random(505)
    cs, zs, ys, ps = [], [], [], []
    for _ in range(9):
        f = [rnd.randrange(R) for _ in range(4)]
        z = rnd.randrange(R)
        y, p = setup.proof(f, z, 2)
        cs.append(setup.commit(f, 2)); zs.append(z); ys.append(y); ps.append(p)
    bad = 4
    ys_bad = list(ys); ys_bad[bad] = (ys[bad] + 1) % R
    blobs = [setup.blob_case([rnd.randrange(R) for _ in range(64)], 6) for _ in range(3)]
    cases = {'commitments': [c.hex() for c in cs], 'proofs': [p.hex() for p in ps], 'zs': ['%064x' % z for z in zs], 'ys': ['%064x' % y for y in ys],
             'ys_bad': ['%064x' % y for y in ys_bad], 'bad': bad, 'tau': setup.tau_g2().hex(), 'seed': bytes(range(32)).hex(),
             'blobs': [b[0].hex() for b in blobs], 'blob_commitments': [b[1].hex() for b in blobs], 'blob_proofs': [b[2].hex() for b in blobs]}
    del eng
    path = tmp_path / 'kzg_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_kzg.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS KZG ok' in out.stdout, out.stdout + out.stderr
