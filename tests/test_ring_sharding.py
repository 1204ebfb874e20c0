"""figure_2_sweep(scores=True) over two ranks on the CPU (gloo, tests/comm_gloo.py standing in for sharding.RcclComm): every rank
scores its own shard, the score arrays travel through comm.gather beside the estimates and come back in task order on rank 0 -- with
objects of two shapes, so the ranks' score arrays differ in length per task.  The device is replaced by a stand-in whose estimates
and scores encode the task."""
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # comm_gloo, also in the spawned workers


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake(sweep, objects, psf_sets, n_rings):
    ids = sweep.object_ids(objects)

    def estimate(o, p, s):
        return np.full(objects[o].shape[-2:], 100.0 * ids[o] + 10.0 * len(psf_sets[p]) + s)

    def score(o, p, s):
        R = min(objects[o].shape[-2:]) // 2 if n_rings is None else n_rings
        return (1000.0 * ids[o] + 100.0 * len(psf_sets[p]) + 10.0 * s) + np.arange(R * 5, dtype=np.float64).reshape(R, 5)

    def run_and_score(tasks, objects_, psf_sets_, iterations, total_brightness, dtype, device, n_rings_, **k):
        assert n_rings_ == n_rings
        return [estimate(*t) for t in tasks], [score(*t) for t in tasks]
    return estimate, score, run_and_score


def _worker(rank, world, port, out_path):
    import torch.distributed as dist
    from rescan_line_sted_amd import sweep
    from comm_gloo import GlooComm
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    objects = {'cat': np.zeros((1, 10, 12)), 'rings': np.zeros((1, 8, 8)), 'lines': np.zeros((1, 8, 8))}
    psf_sets = {'point': [None], 'line3': [None] * 3}
    for n_rings in (None, 3):
        estimate, score, sweep.run_and_score_tasks = _fake(sweep, objects, psf_sets, n_rings)
        tasks, est, scores = sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 1, 2), iterations=5, comm=GlooComm(dist), scores=True,
                                                  n_rings=n_rings)
        if rank == 0:
            assert len(tasks) == len(est) == len(scores) == 18
            for t, e, s in zip(tasks, est, scores):
                assert np.array_equal(e, estimate(*t)) and np.array_equal(s, score(*t))
            if n_rings is None:
                assert {np.shape(s) for s in scores} == {(4, 5), (5, 5)}          # 8 x 8 and 10 x 12 images
            else:
                assert np.asarray(scores).shape == (18, 3, 5)
        else:
            assert est is None and scores is None
    if rank == 0:
        open(out_path, 'w').write('ok')
    dist.barrier()
    dist.destroy_process_group()


def test_scored_sweep_world_size_2_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / 'ok.txt')
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out).read() == 'ok'


def test_unscored_sweep_keeps_its_signature():
    """scores defaults to False, and the default returns (tasks, estimates) as before."""
    import inspect
    from rescan_line_sted_amd import sweep
    sig = inspect.signature(sweep.figure_2_sweep)
    assert sig.parameters['scores'].default is False and sig.parameters['n_rings'].default is None
    objects, psf_sets = {'a': np.zeros((1, 8, 8))}, {'p': [None]}
    keep = sweep.run_tasks
    sweep.run_tasks = lambda tasks, objects_, *a, **k: [np.full((8, 8), float(s)) for _, _, s in tasks]
    try:
        out = sweep.figure_2_sweep(objects, psf_sets, seeds=(4, 5), iterations=1)
    finally:
        sweep.run_tasks = keep
    assert len(out) == 2 and out[1].shape == (2, 8, 8) and out[1][1, 0, 0] == 5.0
