"""Manual helper (not a test): A/B of one run-time switch on BASELINE config 4 (the figure-2 sweep, 1152 tasks as bench.py's
fig2_sweep leg runs them) in ONE process, interleaved rounds; each configuration keeps a plan cache of its own.

    python3 tools/gpu/sweep_env_ab.py [NAME [VALUE_A VALUE_B]]        (default: RLSTED_SHARE_OBJECTS 0 1)
"""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rescan_line_sted_amd import sweep  # noqa: E402

NAME = sys.argv[1] if len(sys.argv) > 1 else 'RLSTED_SHARE_OBJECTS'
VALUES = tuple(sys.argv[2:4]) if len(sys.argv) > 3 else ('0', '1')
objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
objects = {n: objs[n][0].astype(np.float64) for n in ('astronaut', 'cat', 'lines', 'rings')}
psf_sets = bench.fig2_psf_sets(False)
tasks = sweep.make_tasks(objects, psf_sets, range(16))
shards, costs = sweep.shard_sweep(tasks, objects, psf_sets, bench.K_ITERS, 1)
tasks = [tasks[i] for i in shards[0]]      # grouped by plan, as bench.py's fig2_sweep leg runs them
store, flats = {}, {}
for cfg in VALUES:
    os.environ[NAME] = cfg
    sweep._plans = {}
    res = sweep.run_tasks_device(tasks, objects, psf_sets, bench.K_ITERS, 5e10, 'f32', 0)
    flats[cfg] = np.concatenate([e.ravel() for e in res.download()])
    res.free()
    store[cfg] = sweep._plans
    print('%s=%s: object classes of the first plans: %s' % (NAME, cfg, [p.object_classes() for p in list(store[cfg].values())[:4]]), flush=True)
del os.environ[NAME]
print('estimates identical:', np.array_equal(flats[VALUES[0]], flats[VALUES[1]]), flush=True)
times = {v: [] for v in VALUES}
for r in range(15):
    for cfg in VALUES:
        sweep._plans = store[cfg]
        t0 = time.perf_counter()
        res = sweep.run_tasks_device(tasks, objects, psf_sets, bench.K_ITERS, 5e10, 'f32', 0)
        times[cfg].append(time.perf_counter() - t0)
        res.free()
for cfg in VALUES:
    t = np.array(times[cfg]) * 1e3
    print('%s=%s  %d tasks  median %.3f ms  min %.3f ms  max %.3f ms  rounds %s' % (
        NAME, cfg, len(tasks), np.median(t), t.min(), t.max(), np.round(t, 3).tolist()), flush=True)
