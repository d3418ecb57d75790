"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and none of the --full objects, --steps sets the timed steps, and the
dumped outputs of the last timed step are the oracle's pairings of SURVEY 8(d)'s item stream (the bench inputs, rebuilt here on the host).  The size cap of
the dump is checked on the host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_is_exact_and_capped(tmp_path):
    import torch
    import bench
    n = 4096
    t = torch.randint(0, 256, (576 * n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path / 'a'), 'pairings', t, n)
    a = np.load(tmp_path / 'a' / 'pairings.npy')
    assert a.dtype == np.float32 and a.shape == (n, 576) and (a == t.numpy().reshape(n, 576)).all()
    n = 40000      # 88 MB as float32: a fixed, seeded sample of rows, their indices beside them
    t = torch.randint(0, 256, (576 * n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), 'pairings', t, n)
    files = sorted(os.listdir(tmp_path / 'b'))
    assert files == ['pairings.npy', 'pairings_rows.npy']
    assert sum(os.path.getsize(tmp_path / 'b' / f) for f in files) <= 64 << 20
    rows = np.load(tmp_path / 'b' / 'pairings_rows.npy')
    a = np.load(tmp_path / 'b' / 'pairings.npy')
    assert rows.dtype == np.float64 and len(rows) == len(a) and (np.diff(rows) > 0).all()
    assert (a == t.numpy().reshape(n, 576)[rows.astype(np.int64)]).all()
    assert all((np.load(tmp_path / 'b' / f) == np.load(tmp_path / 'c' / f)).all() for f in files)


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path, oracle):
    import bench
    n, steps = 256, 5
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2', '--batch', str(n), '--inflight', '3',
           '--dump-outputs', str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-3000:]
    line = json.loads(lines[0])
    assert (line['metric'], line['unit'], line['higher_is_better'], line['dtype']) == ('pairings/sec', 'pairings/s', True, 'int64')
    assert line['steps'] == steps and line['warmup'] == 2 and line['full'] is False
    assert line['value'] > 0 and abs(line['value'] * line['ms_per_step'] * 1e-3 - n) < 1e-3 * n      # value = n pairings per timed step
    assert not {'roofline', 'cpu_baseline', 'single_call', 'steady_state', 'product', 'verify_batch', 'config3'} & set(line)
    assert sorted(os.listdir(tmp_path)) == ['pairings.npy']
    a = np.load(tmp_path / 'pairings.npy')
    assert a.dtype == np.float32 and a.shape == (n, 576)
    idx = (0, 1, n // 2, n - 1)
    g1, g2 = oracle.g1_generator(), oracle.g2_generator()
    G1 = b''.join(oracle.g1_mul(g1, bench.bench_scalar(0x6e626c73, 2 * i))[1] for i in idx)
    G2 = b''.join(oracle.g2_mul(g2, bench.bench_scalar(0x6e626c73, 2 * i + 1))[1] for i in idx)
    ref, _ = oracle.pairing_batch(G1, G2, True, False)
    assert a[list(idx)].astype(np.uint8).tobytes() == ref
