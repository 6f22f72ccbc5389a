"""``python bench.py --gpus 2`` launches itself as two ranks (torch.distributed.run, 127.0.0.1) - here in --dry mode on
CPU with gloo: the same launcher, process group, layer buckets of the flat gradient buffer, all-reduce schedule and
JSON line as on the GPUs, around a stub step whose summed gradients are checked on every rank."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _run(*extra, **env_extra):
    env = dict(os.environ, OMP_NUM_THREADS='4', **env_extra)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(REPO / 'bench.py'), '--dry', '--steps', '2', '--warmup', '1', *extra],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(REPO))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout          # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_self_launch_two_ranks_bucketed_allreduce():
    out = _run('--gpus', '2', '--full')
    assert out['n_gpus'] == 2 and out['dry'] is True and out['steps'] == 2
    assert out['config']['parallelism'] == 'dp2' and out['config']['global_batch'] == 64
    r = out['rccl']
    assert r['world_size'] == 2 and r['overlap_allreduce'] is True
    assert r['schedule']['used'] == 'overlap' and set(r['schedule']['probe_ms_per_step']) == {'overlap', 'no_overlap'}
    # PIT model: three BLSTM layers and two linears -> five layer buckets covering all 23 480 914 parameters
    assert len(r['buckets']) == 5 and sum(r['buckets']) == 23480914 and r['flat_gradient_bytes'] == 4 * 23480914
    assert out['value'] > 0 and out['unit'] == 'frames/s'
    # what the first real SCALE record is read against: every bucket's own all-reduce, and the efficiency fields (the dry run has no
    # step without exchange to relate them to)
    assert len(r['bucket_all_reduce_ms']) == 5 and all(t > 0 for t in r['bucket_all_reduce_ms'])
    assert set(r['scaling']) == {'ms_per_step_without_exchange', 'measured_efficiency', 'predicted_efficiency_unoverlapped',
                                 'predicted_efficiency_fully_overlapped'}


def test_recurrence_timeout_falls_back_to_the_unoverlapped_schedule():
    """a watchdog timeout of a persistent recurrence kernel while the bucketed all-reduce runs beside it must not
    end the multi-GPU run: every rank raises in the same step (simulated here in the stub step), bench.py reruns with one
    all-reduce in optimizer_step and says so."""
    out = _run('--gpus', '2', PTMI_BENCH_FAKE_TIMEOUT='1')
    sched = out['rccl']['schedule']
    assert sched['used'] == 'no_overlap' and sched['probe_ms_per_step']['overlap'] is None
    assert sched['probe_ms_per_step']['no_overlap'] > 0 and any('timeout' in n for n in sched['notes'])
    assert out['rccl']['overlap_allreduce'] is False and out['value'] > 0


def test_c4_micro_steps_single_allreduce_per_optimizer_step():
    out = _run('--gpus', '2', '--config', 'c4', '--no-overlap-allreduce')
    assert out['config']['global_batch'] == 64 * 2 * 4 and out['rccl']['overlap_allreduce'] is False
    assert out['config']['frames_per_step'] == 2 * 4 * 64 * 503


def test_single_process_dry():
    out = _run()
    assert out['n_gpus'] == 1 and 'rccl' not in out


def test_plain_run_leaves_the_side_measurements_to_full():
    """A plain run does what the headline needs: the schedule it timed and the bucket layout, no all-reduce timings and no step
    without the exchange (those come with --full)."""
    out = _run('--gpus', '2')
    assert out['n_gpus'] == 2 and out['value'] > 0 and out['ms_per_step'] > 0 and out['steps'] == 2 and out['warmup'] == 1
    r = out['rccl']
    assert r['world_size'] == 2 and r['schedule']['used'] == 'overlap' and sum(r['buckets']) == 23480914
    assert not {'blocking_all_reduce_ms', 'bucket_all_reduce_ms', 'scaling', 'bus_bandwidth_gbs', 'expected'} & set(r), sorted(r)
    assert 'cpu_baseline' not in out


def test_dump_outputs_are_float_arrays_within_budget_and_repeat(tmp_path):
    """``--dump-outputs DIR``: the last timed step's arrays as DIR/<name>.npy, float32 / float64, 64 MB at most in all (the 23.5 M
    parameters of the PIT model are a seeded sample), the same from run to run; ``steps`` and ``ms_per_step`` as without it."""
    import numpy as np
    runs = []
    for name in ('a', 'b'):
        out = _run('--steps', '3', '--dump-outputs', str(tmp_path / name))
        assert out['steps'] == 3 and out['ms_per_step'] > 0
        files = sorted((tmp_path / name).glob('*.npy'))
        assert len(files) == out['dump_outputs']['arrays'] > 0
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        arrays = {f.name: np.load(f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert 'param.linear2.weight.npy' in arrays
        runs.append(arrays)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
