"""`python bench.py --gpus N` launches its own ranks (reference: scripts/flow_training.py:125-128 fans out from one
command with `devices=args.gpus`).  Checked here without a GPU through the dry-run mode (MPC_BENCH_DRYRUN=1: the same
fan-out, process group, barriers and MAX/SUM reductions over gloo with an empty step).  Also the plain run's contract
(headline only, exactly --steps timed steps) and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(env_extra)
    return subprocess.run([sys.executable, 'bench.py'] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus_2_without_rank_env_launches_two_ranks():
    r = _run(['--gpus', '2', '--steps', '3', '--warmup', '1'], {'MPC_BENCH_DRYRUN': '1'})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['ranks_counted'] == 2 and d['config']['parallelism'] == 'dp2'
    assert d['dry_run'] is True and d['value'] == 0.0        # a dry run can never pass for a measurement


def test_world_size_must_match_gpus():
    # a rank environment whose WORLD_SIZE disagrees with --gpus is an error, not a silent 1-GPU run
    r = _run(['--gpus', '4', '--steps', '1', '--warmup', '0'],
             {'MPC_BENCH_DRYRUN': '1', 'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '1'})
    assert r.returncode != 0 and 'WORLD_SIZE=1' in (r.stderr + r.stdout)


def test_more_gpus_than_visible_is_refused_by_the_parent():
    # no dry run: the parent counts the devices and refuses (it starts no rank)
    import torch
    if torch.cuda.device_count() >= 64:
        return
    r = _run(['--gpus', '64', '--steps', '1', '--warmup', '0'], {})
    assert r.returncode != 0 and 'GPU(s) visible' in (r.stderr + r.stdout)


def test_failing_rank_fails_the_parent():
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0', '--workload', 'C2'],
             {'MPC_BENCH_BACKEND': 'gloo'}, timeout=600)           # ranks need a GPU: here they exit non-zero
    import torch
    if not torch.cuda.is_available():
        assert r.returncode != 0


def test_dump_outputs_is_seeded_and_bounded(tmp_path):
    # --dump-outputs: scalars and small arrays as they are; an array larger than its share of the budget as the same seeded sample every time
    import numpy as np
    import torch
    import bench
    big = bench.DUMP_BYTES // 4 + 1000                           # float32 elements: more than one array's share of two
    arrays = {'loss': torch.tensor(1.25), 'small': torch.arange(12.).reshape(3, 4), 'a': torch.randn(big), 'b': torch.randn(big)}
    for d in ('x', 'y'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    names = sorted(os.listdir(tmp_path / 'x'))
    assert names == ['a_sample.npy', 'b_sample.npy', 'loss.npy', 'small.npy']
    assert sum(os.path.getsize(tmp_path / 'x' / n) for n in names) <= bench.DUMP_BYTES + 4096
    for n in names:
        x, y = np.load(tmp_path / 'x' / n), np.load(tmp_path / 'y' / n)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert np.load(tmp_path / 'x' / 'loss.npy').shape == () and np.array_equal(np.load(tmp_path / 'x' / 'small.npy'), arrays['small'].numpy())
    a = np.load(tmp_path / 'x' / 'a_sample.npy')
    assert np.isin(a, arrays['a'].numpy()).all()


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    # a plain run prints the headline only, times exactly --steps steps and writes what its last timed step returned
    import numpy as np
    r = _run(['--gpus', '1', '--steps', '3', '--warmup', '1', '--workload', 'C2', '--dump-outputs', str(tmp_path)], {}, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and d['value'] > 0 and d['unit'] == 'Mevents/s' and d['dtype'] == 'f32'
    assert not {'roofline', 'also', 'cpu_baseline', 'blocks_ms_per_step', 'loss_check'} & set(d)
    files = sorted(os.listdir(tmp_path))
    assert files == ['focus_loss.npy', 'iwes.npy', 'loss.npy', 'smoothness_loss.npy', 'trajectories_grad.npy']
    assert float(np.load(tmp_path / 'loss.npy')) == d['loss']
    assert np.load(tmp_path / 'iwes.npy').shape == (1, 1, 2, 480, 640)
    g = np.load(tmp_path / 'trajectories_grad.npy')
    assert g.shape == (1, 16, 120 * 160, 2) and np.isfinite(g).all() and np.abs(g).max() > 0
