"""figure_2_sweep(ensemble=True) over two ranks on the CPU (gloo, tests/comm_gloo.py standing in for sharding.RcclComm): every rank
reduces the (object, PSF set) keys of its own shard, only the [6] scalars per key travel through comm.gather beside the estimates,
and rank 0 gets every key once with its own numbers -- with objects of two shapes, with and without scores.  The device is
replaced by a stand-in whose estimates, scores and scalars encode the task.  And the refusal of a partition that splits a key."""
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # comm_gloo, also in the spawned workers


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake(sweep, objects, psf_sets, want_scores):
    ids = sweep.object_ids(objects)

    def estimate(o, p, s):
        return np.full(objects[o].shape[-2:], 100.0 * ids[o] + 10.0 * len(psf_sets[p]) + s)

    def score(o, p, s):
        R = min(objects[o].shape[-2:]) // 2
        return (1000.0 * ids[o] + 100.0 * len(psf_sets[p]) + 10.0 * s) + np.arange(R * 5, dtype=np.float64).reshape(R, 5)

    def scalars(o, p, n):
        return np.array([n, ids[o], len(psf_sets[p]), 0.5 * ids[o], 7.0, -1.0])

    def run(tasks, objects_, psf_sets_, iterations, total_brightness, dtype, device, scores, n_rings, **k):
        assert scores == want_scores and k['n_sectors'] is None
        keys, members = sweep.ensemble_keys(tasks)
        return ([estimate(*t) for t in tasks], [score(*t) for t in tasks] if scores else None, keys,
                np.stack([scalars(o, p, len(m)) for (o, p), m in zip(keys, members)]))
    return estimate, score, scalars, run


def _worker(rank, world, port, out_path):
    import torch.distributed as dist
    from rescan_line_sted_amd import sweep
    from comm_gloo import GlooComm
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    objects = {'cat': np.zeros((1, 10, 12)), 'rings': np.zeros((1, 8, 8)), 'lines': np.zeros((1, 8, 8))}
    psf_sets = {'point': [None], 'line3': [None] * 3}
    for want_scores in (False, True):
        estimate, score, scalars, sweep.run_score_reduce_tasks = _fake(sweep, objects, psf_sets, want_scores)
        got = sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 1, 2), iterations=5, comm=GlooComm(dist), scores=want_scores,
                                   ensemble=True)
        assert len(got) == (4 if want_scores else 3)
        tasks, est, ens = got[0], got[1], got[-1]
        if rank == 0:
            assert len(tasks) == len(est) == 18
            for t, e in zip(tasks, est):
                assert np.array_equal(e, estimate(*t))
            if want_scores:
                for t, s in zip(tasks, got[2]):
                    assert np.array_equal(s, score(*t))
            keys, sc = ens
            assert sorted(keys) == sorted({(o, p) for o, p, _ in tasks}) and len(keys) == 6 and sc.shape == (6, 6)
            for (o, p), row in zip(keys, sc):
                assert np.array_equal(row, scalars(o, p, 3)), (o, p)
        else:
            assert est is None and ens is None and (not want_scores or got[2] is None)
    if rank == 0:
        open(out_path, 'w').write('ok')
    dist.barrier()
    dist.destroy_process_group()


def test_ensemble_sweep_world_size_2_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / 'ok.txt')
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out).read() == 'ok'


def test_a_partition_that_splits_a_key_is_refused(monkeypatch):
    """Seeds 0 and 1 of ('rings', 'point') on rank 0, seed 2 on rank 1: ValueError naming the key, before anything runs; the same
    partition without ensemble=True is none of this function's business."""
    from rescan_line_sted_amd import sweep
    objects = {'rings': np.zeros((1, 8, 8))}
    psf_sets = {'point': [None]}

    class TwoRanks:
        world, rank = 2, 0

    def split(tasks, objects_, psf_sets_, iterations, world):
        return [[0, 1], [2]], [1.0] * len(tasks)

    def never(*a, **k):
        raise AssertionError('the sweep ran')
    monkeypatch.setattr(sweep, 'shard_sweep', split)
    monkeypatch.setattr(sweep, 'run_score_reduce_tasks', never)
    monkeypatch.setattr(sweep, 'run_tasks', never)
    with pytest.raises(ValueError, match=r"\('rings', 'point'\)"):
        sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 1, 2), iterations=1, comm=TwoRanks(), ensemble=True)
