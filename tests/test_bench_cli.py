"""bench.py's N > 1 control flow on a box without GPUs (RLSTED_BENCH_STUB=1 swaps the device plan for a
stand-in and RCCL for gloo): `--gpus N` launches N ranks by itself, the ranks agree on n_gpus, the gather
delivers N x B frames, and exactly one JSON line comes out.  A plain run carries the headline alone (--full adds the
rest), and --dump-outputs writes the same seeded sample of the last step's outputs in every run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _env():
    env = dict(os.environ, RLSTED_BENCH_STUB='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    return env


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_line(stdout):
    lines = [ln for ln in stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_gpus_2_launches_two_ranks_by_itself():
    r = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '4', '--full'],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = _one_line(r.stdout)
    assert d['n_gpus'] == 2 and d['steps'] == 2 and d['scaling'] == 'weak'
    assert d['final_gather']['frames_on_root'] == 2 * 4
    assert d['value'] > 0 and 'roofline' in d
    # N > 1, --full: the line also carries BASELINE config 4 through the sharder (cost-weighted partition, one gather on rank 0)
    sw = d['fig2_sweep']
    assert sw['tasks'] == 1152 and sw['frames_on_root'] == 1152 and sum(sw['tasks_per_rank']) == 1152
    # by plan group: the 36 (PSF set, shape) groups are dealt whole, so no plan is set up on two ranks
    assert sum(sw['groups_per_rank']) == 36 and max(sw['cost_per_rank_rel']) < 1.1 and sw['gather_ms'] >= 0
    assert 'broadcast' in sw['psf_sets'] or 'every rank' in sw['psf_sets']


def test_under_the_drivers_launcher_command():
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), BENCH, '--gpus', '2', '--steps', '1', '--warmup', '0', '--batch', '2']
    r = subprocess.run(cmd, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = _one_line(r.stdout)
    assert d['n_gpus'] == 2 and d['final_gather']['frames_on_root'] == 4


def test_rank_count_mismatch_is_an_error():
    env = dict(_env(), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--steps', '1', '--warmup', '0'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b'--gpus 2' in r.stderr


HEADLINE_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup')
FULL_ONLY_KEYS = ('roofline', 'accuracy', 'cpu_baseline', 'fig2_sweep', 'size_2048', 'line_rescan_512', 'f64_512')


def _bench(args, env, timeout=120):
    r = subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return _one_line(r.stdout)


def test_plain_run_times_its_steps_and_nothing_else():
    """A plain run: set-up, warm-up, the K timed steps, the line -- the figures of --full are not in it.  The stand-in plan
    sleeps 2 ms per step, so ms_per_step says that --steps set the number of steps timed."""
    d = _bench(['--gpus', '1', '--steps', '5', '--warmup', '1', '--batch', '4'], _env())
    assert all(k in d for k in HEADLINE_KEYS), d
    assert d['steps'] == 5 and d['unit'] == 'frames/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert 2.0 <= d['ms_per_step'] < 1000.0
    assert abs(d['value'] - 4 * 1e3 / d['ms_per_step']) < 1e-6 * d['value']
    assert not [k for k in FULL_ONLY_KEYS if k in d], d


def test_full_run_carries_the_roofline():
    d = _bench(['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '4', '--full'], _env())
    assert d['steps'] == 2 and d['roofline']['frames_per_launch'] == 4 and d['roofline']['unit'] == 'GB/s'


def test_steps_below_one_is_an_error():
    r = subprocess.run([sys.executable, BENCH, '--steps', '0'], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b'--steps' in r.stderr


def test_dump_outputs_writes_the_same_sample_every_run(tmp_path):
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    for out in (a, b):
        d = _bench(['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '3', '--dump-outputs', out], _env())
        assert 'roofline' not in d
    for name, shape in (('estimate', (3, 512, 512)), ('measurement', (3, 1, 512, 512))):
        x, y = np.load(os.path.join(a, name + '.npy')), np.load(os.path.join(b, name + '.npy'))
        assert x.shape == shape and x.dtype == np.float32 and np.array_equal(x, y)


def test_dump_sample_stays_within_its_budget(tmp_path, monkeypatch):
    """The sample of a large batch: seeded frames, the same ones in both files; a frame larger than its share of the
    budget becomes a seeded sample of its pixels."""
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 5 * 32 * 32 * 4 * 3)         # three frames of one estimate + four views
    plan = bench.StubPlan([np.ones((1, 3, 3))] * 4, 50, 32, 32)
    plan._est = np.random.default_rng(3).random((50, 32, 32))
    bench.dump_outputs(plan, str(tmp_path / 'a'), stub=True)
    est = np.load(str(tmp_path / 'a' / 'estimate.npy'))
    frames = bench.dump_frames(50, 5 * 32 * 32 * 4)
    assert len(frames) == 3 and list(frames) == sorted(set(frames)) and np.array_equal(frames, bench.dump_frames(50, 5 * 32 * 32 * 4))
    assert est.dtype == np.float32 and np.array_equal(est, plan._est[frames].astype(np.float32))
    assert np.load(str(tmp_path / 'a' / 'measurement.npy')).shape == (3, 4, 32, 32)
    monkeypatch.setattr(bench, 'DUMP_BYTES', 5 * 32 * 32 * 4 // 2)        # not even one frame: pixels of frame dump_frames(...)[0]
    bench.dump_outputs(plan, str(tmp_path / 'b'), stub=True)
    est, meas = np.load(str(tmp_path / 'b' / 'estimate.npy')), np.load(str(tmp_path / 'b' / 'measurement.npy'))
    assert est.shape == (1, bench.DUMP_BYTES // 5 // 4) and meas.shape == (1, bench.DUMP_BYTES * 4 // 5 // 4)
    assert est.nbytes + meas.nbytes <= bench.DUMP_BYTES
    f, = bench.dump_frames(50, 5 * 32 * 32 * 4)
    assert np.all(np.isin(est[0], plan._est[f].astype(np.float32)))


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_timed_step(tmp_path):
    """On the device: the files --dump-outputs writes hold the estimate and the measurement of the LAST timed step (its seed:
    warm-up + steps - 1), bit for bit what simulate + 20 iterations of the same batch leave."""
    from rescan_line_sted_amd import _lib
    import bench
    env = dict(_env())
    env.pop('RLSTED_BENCH_STUB')
    out = str(tmp_path / 'dump')
    d = _bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '6', '--dump-outputs', out], env, timeout=600)
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and 'roofline' not in d
    obj, psf, brightness, _ = bench.workload(512)
    plan = _lib.DeconvPlan(psf, 6, 512, 512, dtype='f32')
    plan.set_object(np.broadcast_to(obj, (6, 512, 512)), brightness)
    plan.simulate(seed=1 + 3 - 1)
    plan.iterate(bench.K_ITERS)
    frames = bench.dump_frames(6, 2 * 512 * 512 * 4)
    assert list(frames) == list(range(6))
    est, meas = np.load(os.path.join(out, 'estimate.npy')), np.load(os.path.join(out, 'measurement.npy'))
    assert est.dtype == np.float32 and meas.dtype == np.float32
    assert np.array_equal(est.astype(np.float64), plan.estimate()[frames])
    assert np.array_equal(meas.astype(np.float64), plan.measurement()[frames])
