"""The facade's PointG2.combineShares / PointG1.combineShares / combineSharesBatch on the GPU, on the reference-made threshold cases (tests/js/test_threshold.js)."""
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'noble-bls12-381_amd', 'js')
needs_node = pytest.mark.skipif(shutil.which('node') is None or not os.path.exists('/usr/include/node/node_api.h'), reason='node / N-API headers not available')


@needs_node
@pytest.mark.gpu
def test_threshold_facade_on_gpu():
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-D_GNU_SOURCE', '-I/usr/include/node', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(JS, 'nbls_napi.c'), '-o', os.path.join(JS, 'nbls_napi.node'), '-ldl'])
    out = subprocess.run(['node', os.path.join(ROOT, 'tests', 'js', 'test_threshold.js')], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'JS threshold recombination ok' in out.stdout, out.stdout + out.stderr
