"""Manual helper (not a test): the run of tools/gpu/sweep_env_ab.py -- the figure-2 sweep, BASELINE config 4, 1152 tasks -- as an
A/B of two LIBRARIES in one process, interleaved rounds; each library has its own binding (tools/gpu/ab_bench.py bind), its own
copy of the sweep module and its own plan cache.

    python3 tools/gpu/sweep_lib_ab.py LIB_A LIB_B
"""
import os
import sys
import time
import types

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import ab_bench  # noqa: E402
import rescan_line_sted_amd  # noqa: E402,F401
# (quality and sharding keep the package's own binding: made here, before bind() points RLSTED_LIB at a library that may be older than
# the binding's prototypes)
import rescan_line_sted_amd._lib  # noqa: E402,F401

libs = sys.argv[1:3]
sweeps = []
for i, path in enumerate(libs):
    ab_bench.bind(path, str(i))
    src = open(os.path.join(ROOT, 'rescan_line_sted_amd', 'sweep.py')).read()
    assert 'from ._lib import' in src
    src = src.replace('from ._lib import', 'from ._lib_%d import' % i)
    m = types.ModuleType('rescan_line_sted_amd.sweep_%d' % i)
    m.__package__ = 'rescan_line_sted_amd'
    m.__file__ = os.path.join(ROOT, 'rescan_line_sted_amd', 'sweep.py')
    sys.modules[m.__name__] = m
    exec(compile(src, m.__file__, 'exec'), m.__dict__)
    sweeps.append(m)

objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
objects = {n: objs[n][0].astype(np.float64) for n in ('astronaut', 'cat', 'lines', 'rings')}
psf_sets = bench.fig2_psf_sets(False)
sweep = sweeps[0]
tasks = sweep.make_tasks(objects, psf_sets, range(16))
shards, costs = sweep.shard_sweep(tasks, objects, psf_sets, bench.K_ITERS, 1)
tasks = [tasks[i] for i in shards[0]]
flats = []
for m in sweeps:
    res = m.run_tasks_device(tasks, objects, psf_sets, bench.K_ITERS, 5e10, 'f32', 0)
    flats.append(np.concatenate([e.ravel() for e in res.download()]))
    res.free()
    print('%s: %d plans' % (m.__name__, len(m._plans)), flush=True)
print('estimates identical:', np.array_equal(flats[0], flats[1]), flush=True)
times = [[] for _ in sweeps]
for r in range(15):
    for i, m in enumerate(sweeps):
        t0 = time.perf_counter()
        res = m.run_tasks_device(tasks, objects, psf_sets, bench.K_ITERS, 5e10, 'f32', 0)
        times[i].append(time.perf_counter() - t0)
        res.free()
for i, path in enumerate(libs):
    t = np.array(times[i]) * 1e3
    print('%s  %d tasks  median %.3f ms  min %.3f ms  max %.3f ms  spread %.3f ms  rounds %s' % (
        path, len(tasks), np.median(t), t.min(), t.max(), t.max() - t.min(), np.round(t, 3).tolist()), flush=True)
