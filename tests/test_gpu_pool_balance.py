"""nbls_pool_init_ex with NBLS_POOL_BALANCE: a batch goes to the context with the fewest batches outstanding (at most K each, ties round-robin), and a submit waits while
every context is at K.  Depth 4, n = 64, 40 submits, every submit into a buffer of its own (tests/pool_balance_child.py): all 40 buffers equal the oracle's bytes, the slot
nbls_pool_next_slot announces is the slot the submit reports, nbls_pool_outstanding never exceeds K, the same with K = 1, and without the flag the slots are exactly
i mod depth.  Every device case runs in a child process under a time limit: a wait that never ends fails here.  The choice itself is checked on the host
(tests/test_pool_pick.py); the refused settings need no device either."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SUBMITS = 4, 40
ENV_SWITCHES = ('NBLS_POOL_BALANCE', 'NBLS_POOL_MAX_OUTSTANDING', 'NBLS_POOL_SPREAD', 'NBLS_POOL_SPREAD_LEVELS')


def _child(modes, max_outstanding=None):
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    if max_outstanding is not None:
        env['NBLS_POOL_MAX_OUTSTANDING'] = str(max_outstanding)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'pool_balance_child.py')] + list(modes), env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _check_balanced(r, K):
    print(r)
    assert r['buffers'] == SUBMITS and r['differ_from_oracle'] == 0, r
    assert len(r['reported']) == SUBMITS and all(0 <= s < DEPTH for s in r['reported']), r
    assert [a for a in r['announced'] if a is not None] == [s for a, s in zip(r['announced'], r['reported']) if a is not None], r      # announced = used
    assert sum(a is None for a in r['announced']) == SUBMITS // 5, r      # and some submits chose for themselves
    assert r['reported'][:DEPTH] == list(range(DEPTH)), r      # whether or not a batch has retired by then, the first `depth` picks visit every context once, in order
    assert 0 <= r['min_outstanding'] and r['max_outstanding'] <= K, r
    assert r['outstanding_after_sync'] == [0] * DEPTH, r
    assert all(c != 0 for c in r['bad_index']), r


@pytest.fixture(scope='module')
def default_bound():
    return _child(['balance', 'plain'])


@pytest.mark.gpu
def test_balanced_pool_matches_the_oracle_and_announces_the_slot_it_uses(default_bound):
    _check_balanced(default_bound['balance'], 2)


@pytest.mark.gpu
def test_without_the_flag_the_slots_are_round_robin(default_bound):
    r = default_bound['plain']
    assert r['reported'] == [i % DEPTH for i in range(SUBMITS)], r
    assert all(a is None or a == i % DEPTH for i, a in enumerate(r['announced'])), r
    assert r['max_outstanding'] == 0 and r['outstanding_after_sync'] == [0] * DEPTH, r      # no events without the flag
    assert r['differ_from_oracle'] == 0 and r['buffers'] == SUBMITS, r


@pytest.mark.gpu
def test_one_outstanding_per_context_still_completes():
    r = _child(['balance'], max_outstanding=1)
    assert r['max_outstanding_env'] == '1'
    _check_balanced(r['balance'], 1)


def test_refused_settings_need_no_device():
    """NBLS_POOL_MAX_OUTSTANDING outside 1 .. 8 and an unknown flag are NBLS_EINVAL before any device work (the variable is read once per process: a child each)"""
    code = ('import ctypes as C, sys; lib = C.CDLL(sys.argv[1]); h = C.c_void_p(); '
            'print(lib.nbls_pool_init_ex(0, 4, int(sys.argv[2]), C.byref(h)), h.value)')
    lib = os.path.join(ROOT, 'noble-bls12-381_amd', 'libnbls.so')
    base = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    for value, flags in (('0', 2), ('9', 2), ('-1', 2), ('abc', 2), ('9', 0), (None, 4), (None, 7)):
        env = dict(base) if value is None else dict(base, NBLS_POOL_MAX_OUTSTANDING=value)
        p = subprocess.run([sys.executable, '-c', code, lib, str(flags)], env=env, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.split() == ['-1', 'None'], (value, flags, p.stdout, p.stderr[-500:])
