"""The facade's PointG1.groth16ProvingKey / groth16Prove on the GPU (tests/js/test_groth16_prove.js): one proof through the facade equals the Python binding's bytes for the same
(z, r, s), and the facade's verifyGroth16Batch accepts it; the keys are groth16_prove_cases.py's test-only ones."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from groth16_prove_cases import R, family, ProvingKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')
NAMES = {'alpha_g1_48': 'alphaG1', 'beta_g1_48': 'betaG1', 'beta_g2_96': 'betaG2', 'delta_g1_48': 'deltaG1', 'delta_g2_96': 'deltaG2', 'a_query48': 'aQuery',
         'b_g1_query48': 'bG1Query', 'b_g2_query96': 'bG2Query', 'l_query48': 'lQuery', 'h_query48': 'hQuery'}


@needs_node
@pytest.mark.gpu
def test_groth16_prover_facade_on_gpu(tmp_path, oracle):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    rnd = random.Random(1900)
    log2_n, n_free, rows, m = 3, 5, 6, 2
    A, B, Cm, witness = family(log2_n, n_free, rows, rnd)
    n_vars = n_free + rows
    key = ProvingKey(oracle, log2_n, n_vars, m, (A, B, Cm), rnd)
    points = key.points()
    z, r, s = witness(rnd), rnd.randrange(R), rnd.randrange(R)
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    pk = eng.groth16_pk(log2_n, n_vars, m, (A, B, Cm), **points)
    proofs, st = eng.groth16_prove(pk, [z], rs=[(r, s)])
    assert st == [0] and proofs[0] == key.expected_proof(z, r, s)
    pk.close(); eng.close()
    alpha, beta, gamma, delta, ic = key.vk_points()
    hexes = lambda v: v.hex() if isinstance(v, bytes) else [p.hex() for p in v]
    cases = {'log2n': log2_n, 'nVars': n_vars, 'nPublic': m, 'matrices': [[[[c, '%064x' % v] for c, v in row] for row in M] for M in (A, B, Cm)],
             'points': {NAMES[k]: hexes(v) for k, v in points.items()}, 'z': ['%064x' % v for v in z], 'rs': ['%064x' % r, '%064x' % s], 'proof': proofs[0].hex(),
             'vk': {'alpha': alpha.hex(), 'beta': beta.hex(), 'gamma': gamma.hex(), 'delta': delta.hex(), 'ic': [p.hex() for p in ic]}}
    path = tmp_path / 'groth16_prove_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_groth16_prove.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS Groth16 prove ok' in out.stdout, out.stdout + out.stderr
