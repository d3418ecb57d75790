"""The balanced pool's choice as a pure function (csrc/pool_pick.h, NBLS_POOL_BALANCE): tests/c/pool_pick_test.cpp on the host alone -- the fewest outstanding wins, ties go
round-robin behind the context used last (wrap-around included), every context at the bound gives -1, K = 1, depth = 1, and from all-zero counts `depth` picks visit every
context once.  Built once plain and once as a stand-alone program under AddressSanitizer + UBSan.  The device side is tests/test_gpu_pool_balance.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'c', 'pool_pick_test.cpp')
INC = '-I' + os.path.join(ROOT, 'noble-bls12-381_amd', 'csrc')


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == 'ok', p.stderr
    return p


def test_pick_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), 'pool_pick_test')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', INC, SRC, '-o', exe])
    _run(exe)


@pytest.mark.skipif(subprocess.call(['sh', '-c', 'echo "int main(){}" | g++ -x c++ -fsanitize=address,undefined -o /dev/null - 2>/dev/null']) != 0, reason='no sanitizer runtime')
def test_pick_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), 'pool_pick_test_san')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', INC, SRC, '-o', exe])
    p = _run(exe)
    assert 'ERROR: AddressSanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr
