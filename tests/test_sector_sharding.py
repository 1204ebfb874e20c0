"""figure_2_sweep(scores=True, n_sectors=S) over two ranks on the CPU (gloo, tests/comm_gloo.py standing in for sharding.RcclComm):
the (R, S, 5) score arrays travel flat through comm.gather beside the estimates and come back in task order and shape on rank 0 --
with objects of two shapes, so the ranks' score arrays differ in length per task.  The device is replaced by a stand-in whose
estimates and scores encode the task."""
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


def _fake(sweep, objects, psf_sets, n_rings, n_sectors):
    ids = sweep.object_ids(objects)

    def estimate(o, p, s):
        return np.full(objects[o].shape[-2:], 100.0 * ids[o] + 10.0 * len(psf_sets[p]) + s)

    def score(o, p, s):
        R = min(objects[o].shape[-2:]) // 2 if n_rings is None else n_rings
        cell = (R, 5) if n_sectors is None else (R, n_sectors, 5)
        return (1000.0 * ids[o] + 100.0 * len(psf_sets[p]) + 10.0 * s) + np.arange(np.prod(cell), dtype=np.float64).reshape(cell)

    def run_and_score(tasks, objects_, psf_sets_, iterations, total_brightness, dtype, device, n_rings_, n_sectors=None, **k):
        assert n_rings_ == n_rings and n_sectors == want_sectors
        return [estimate(*t) for t in tasks], [score(*t) for t in tasks]
    want_sectors = n_sectors
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
    for n_rings, n_sectors in ((None, 6), (3, 4), (None, 1), (3, None)):
        estimate, score, sweep.run_and_score_tasks = _fake(sweep, objects, psf_sets, n_rings, n_sectors)
        tasks, est, scores = sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 1, 2), iterations=5, comm=GlooComm(dist), scores=True,
                                                  n_rings=n_rings, n_sectors=n_sectors)
        if rank == 0:
            assert len(tasks) == len(est) == len(scores) == 18
            for t, e, s in zip(tasks, est, scores):
                assert np.array_equal(e, estimate(*t)) and np.array_equal(s, score(*t))
            if n_rings is None:
                assert {np.shape(s) for s in scores} == {(4, n_sectors, 5), (5, n_sectors, 5)}     # 8 x 8 and 10 x 12 images
            elif n_sectors is None:
                assert np.asarray(scores).shape == (18, 3, 5)
            else:
                assert np.asarray(scores).shape == (18, 3, n_sectors, 5)
        else:
            assert est is None and scores is None
    if rank == 0:
        open(out_path, 'w').write('ok')
    dist.barrier()
    dist.destroy_process_group()


def test_sector_scored_sweep_world_size_2_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / 'ok.txt')
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out).read() == 'ok'


def test_pack_stats_keeps_the_sector_axis():
    from rescan_line_sted_amd import sweep
    same = sweep._pack_stats([np.zeros((4, 6, 5)), np.ones((4, 6, 5))])
    assert isinstance(same, np.ndarray) and same.shape == (2, 4, 6, 5)
    mixed = sweep._pack_stats([np.zeros((4, 6, 5)), np.ones((5, 6, 5))])
    assert isinstance(mixed, list) and mixed[1].shape == (5, 6, 5)
