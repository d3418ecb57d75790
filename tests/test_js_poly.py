"""The facade's PointG1.evalCommitment / PointG2.evalCommitment / evalCommitmentBatch on the GPU (tests/js/test_poly.js): bytes, hex and points, G1 and G2, against the bytes the
Python binding's poly_eval gives for the same commitments, plus the thrown error for a coefficient that does not decode."""
import importlib
import json
import os
import random
import shutil
import subprocess
import pytest
from goldenio import hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_eval_commitment_facade_on_gpu(tmp_path, golden):
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    eng = importlib.import_module('noble-bls12-381_amd').Engine(0)
    rnd = random.Random(404)
    cases = {'g1': [], 'g2': []}
    for t, ids in ((3, [1, 2, 3, 4, 5]), (1, [7]), (4, [0, 1, R - 1, R + 2, (1 << 256) - 1, rnd.getrandbits(256)])):
        keys = [rnd.randrange(1, R).to_bytes(32, 'big') for _ in range(t)]
        g1 = eng.get_public_keys(keys)                      # [a_j]G
        g2 = eng.sign_batch([b'commitment base'] * t, keys)   # [a_j]H: a commitment in G2 to the same polynomial
        for side, coefs in (('g1', g1), ('g2', g2)):
            out, st = eng.poly_eval([(coefs, ids)], g2=side == 'g2')
            assert st == [[0] * len(ids)]
            cases[side].append({'coefs': [c.hex() for c in coefs], 'ids': ['%064x' % x for x in ids], 'out': [o.hex() for o in out[0]]})
    # f = a (x - 2): zero at 2
    a = rnd.randrange(1, R)
    coefs = eng.get_public_keys([(-2 * a % R).to_bytes(32, 'big'), a.to_bytes(32, 'big')])
    out, st = eng.poly_eval([(coefs, [1, 2])])
    assert st == [[0, 1]]
    cases['zero'] = {'coefs': [c.hex() for c in coefs], 'ids': [1, 2], 'out': [o.hex() for o in out[0]]}
    cases['g1_sub'] = [v['hex'] for v in golden['codec']['g1'] if 'subgroup' in v['result']][0]
    cases['g2_root'] = [v['hex'] for v in golden['codec']['g2'] if v['result'] == 'Failed to find a square root'][0]
    del eng
    path = tmp_path / 'poly_cases.json'
    path.write_text(json.dumps(cases))
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_poly.js'), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS commitment evaluation ok' in out.stdout, out.stdout + out.stderr
