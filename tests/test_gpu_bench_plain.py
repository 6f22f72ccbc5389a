"""A plain ``bench.py`` run on one GPU: set-up, warm-up, the timed steps, ``--dump-outputs`` and the JSON line - none of the side
measurements that ``--full`` adds behind the timed steps (per-kernel figures, eager / host-to-device / ragged variants, CPU baseline)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def test_plain_run_times_the_captured_step_and_nothing_else(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(REPO / 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '2',
                        '--dump-outputs', str(tmp_path / 'out')],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(REPO))
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, p.stdout[-2000:]
    d = json.loads(line[0])
    assert d['n_gpus'] == 1 and d['steps'] == 4 and d['warmup'] == 2 and d['unit'] == 'frames/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['ms_per_step'] > 0
    assert abs(d['value'] - d['config']['frames_per_step'] / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    assert 'one hipGraph per optimizer step' in d['config']['step_driver']
    side = {'roofline', 'other_kernels', 'roofline_family', 'cpu_baseline', 'ms_per_step_eager_deferred', 'ms_per_step_sync_checks',
            'ms_per_step_h2d', 'value_ragged', 'value_ragged_graph', 'value_to_device_inclusive', 'rccl'}
    assert not side & set(d), sorted(side & set(d))
    files = sorted((tmp_path / 'out').glob('*.npy'))
    assert len(files) == d['dump_outputs']['arrays'] > 0 and (tmp_path / 'out' / 'loss.npy').exists()
