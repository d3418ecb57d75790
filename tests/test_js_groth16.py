"""The facade's PointG1.Groth16Vk / verifyGroth16Batch (and its Async twin) on the GPU (tests/js/test_groth16.js): nine valid proofs and a tampered one from the test-only key
of groth16_cases.py; hex, bytes and packed arrays in."""
import json
import os
import random
import shutil
import subprocess
import pytest
from groth16_cases import R, Key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_groth16_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    rnd = random.Random(707)
    key = Key(oracle, 3, rnd)
    xs = [[rnd.randrange(R) for _ in range(3)] for _ in range(9)]
    proofs = [key.proof_bytes(key.prove(x, rnd)) for x in xs]
    bad = 5
    xs_bad = [list(x) for x in xs]
    xs_bad[bad][1] = (xs_bad[bad][1] + 1) % R
    alpha, beta, gamma, delta, ic = key.vk_points()
    cases = {'alpha': alpha.hex(), 'beta': beta.hex(), 'gamma': gamma.hex(), 'delta': delta.hex(), 'ic': [p.hex() for p in ic], 'proofs': [p.hex() for p in proofs],
             'inputs': [['%064x' % v for v in x] for x in xs], 'inputs_bad': [['%064x' % v for v in x] for x in xs_bad], 'bad': bad, 'seed': bytes(range(32)).hex()}
    path = tmp_path / 'groth16_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_groth16.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS Groth16 ok' in out.stdout, out.stdout + out.stderr
