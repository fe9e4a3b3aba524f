"""bench.py without --full: the headline leg and nothing else - no golden parity although the workload has a golden,
no CPU baseline, no extra legs, no telemetry - and --dump-outputs still writes the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_headline_leg_only(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    d = tmp_path / 'out'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', 'cfg4', '--pairs', '2',
                        '--steps', '2', '--warmup', '1', '--detail', 'stdout', '--dump-outputs', str(d)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith('BENCH_DETAIL ')
    full = json.loads(lines[0][len('BENCH_DETAIL '):])
    c = json.loads(lines[1])
    assert c['value'] > 0 and c['ms_per_step'] > 0 and c['steps'] == 2 and c['warmup'] == 1 and c['dtype'] == 'f16x3'
    assert c['roofline']['achieved'] > 0 and c['end_to_end']['exec_gflop_per_pair'] > 0
    assert c['cpu_baseline'] is None and c['parity'] == {'tolerance': 1e-3}
    assert 'extra' not in full and 'per_rank' not in full and 'solo' not in full
    assert full['host']['telemetry'] is None
    assert sorted(os.listdir(d)) == ['det.npy', 'end.npy', 'link0.npy', 'new.npy', 'pair_index.npy']
    assert np.load(d / 'det.npy').shape == (2, 3, 256) and np.load(d / 'link0.npy').shape == (2, 3, 128, 128)
