"""nbls_pool_init_ex with NBLS_POOL_SPREAD_PRIORITIES: a pool deeper than the hardware queues in force creates its contexts' streams round-robin over the device's stream
priority levels (the runtime's GPU_MAX_HW_QUEUES is a limit per priority level), plain nbls_pool_init and pools that fit the queues keep default-priority streams, and the
bytes do not depend on the placement.  The queue cap is read when the runtime initialises, so every device case runs tests/pool_priorities_child.py in a fresh process;
the level assignment itself (one priority level included) is checked on the host alone (tests/c/pool_levels_test.cpp)."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(mode, depth, queues='4'):
    env = {k: v for k, v in os.environ.items() if k not in ('NBLS_KEEP_HW_QUEUES', 'NBLS_POOL_SPREAD', 'NBLS_POOL_SPREAD_LEVELS')}
    env['GPU_MAX_HW_QUEUES'] = queues
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'pool_priorities_child.py'), mode, str(depth)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


@pytest.mark.gpu
def test_flag_on_cap_of_four_spreads_twelve_streams_and_keeps_the_bytes():
    r, err = _child('ex', 12)
    print(r)
    L = r['levels']
    least, greatest = r['priority_range']
    per_level = Counter(r['priorities'])
    assert len(r['priorities']) == 12 and all(greatest <= p <= least for p in r['priorities']), r
    assert len(per_level) == min(L, 3), r      # the pool spreads over up to three levels: all of them in use
    if L == 1:
        assert per_level == {0: 12}, r
    if L >= 3:
        assert max(per_level.values()) <= 4, r      # at most four streams (= the queues of a level) on a level
        assert 'hardware queues' not in err      # twelve streams, twelve queues: nothing to warn about
    # 3 rounds x 12 contexts at n = 7 and n = 257, every buffer against a one-context nbls_pairing_batch_dev and against the oracle
    assert r['compared'] == 24 and r['differ_from_single'] == 0 and r['differ_from_oracle'] == 0, r


@pytest.mark.gpu
def test_flag_on_depth_four_keeps_the_default_priority():
    r, err = _child('ex', 4)
    assert r['priorities'] == [0] * 4, r
    assert 'hardware queues' not in err


@pytest.mark.gpu
def test_plain_init_keeps_the_default_priority_and_warns():
    r, err = _child('plain', 12)
    assert r['priorities'] == [0] * 12, r
    assert r['bad_index'][0] != 0 and r['bad_index'][1] != 0, r
    assert 'hardware queues' in err


def test_level_assignment_on_the_host(tmp_path):
    """pool_levels.h without a device: one priority level, pools that fit the queues, twelve on four, a cap of two levels, depths beyond levels x queues"""
    exe = os.path.join(str(tmp_path), 'pool_levels_test')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-I' + os.path.join(ROOT, 'noble-bls12-381_amd', 'csrc'), os.path.join(ROOT, 'tests', 'c', 'pool_levels_test.cpp'), '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == 'ok', p.stderr
