#!/usr/bin/env python3
"""What iteration checkpoints cost and save on BASELINE config 4's 1152 tasks (manual study), f32, save
points 1 2 5 10 20 50 100:

  loop         the curve as one sweep per K (sweep._bias_variance_one_sweep_per_k): sum(K) = 188 iterations per task
  curve        sweep.bias_variance_vs_iterations: one sweep of 100 iterations with 7 checkpoints, each reduced on the device
  plain        sweep.run_tasks_device, 100 iterations: no checkpoint
  ck7          sweep.run_tasks_checkpoints_device at the 7 save points, estimates and trace
  trace7       ... trace only
  trace_all    ... trace only, at every iteration 1 .. 100
  sweep20      sweep.run_tasks_device, 20 iterations: the device part of the plain figure_2_sweep

warmed, alternated in one process, --repeats times each, a host clock around calls that end in a synchronise.  Prints every time,
the medians, loop / curve, and the checkpoints' share of a run: (ck7 - plain) / ck7 and (trace_all - plain) / trace_all.
--copy adds a device-to-device hipMemcpy of the bytes one checkpoint of all tasks moves.  --only ROUTE[,ROUTE] restricts the routes
(a trace run under rocprofv3 wants few launches).

    python tools/gpu/checkpoint_bench.py [--repeats 5] [--only plain,ck7] [--copy] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ring_stats_bench import BRIGHT, workload          # noqa: E402

SAVE_POINTS = [1, 2, 5, 10, 20, 50, 100]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default=None)
    ap.add_argument('--copy', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    log = open(a.out, 'a') if a.out else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()
    from rescan_line_sted_amd import sweep
    objects, psf_sets, seeds, _ = workload('config4')
    tasks = sweep.make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    keys = sweep.ensemble_keys(tasks)[0]
    have_ck = hasattr(sweep, 'run_tasks_checkpoints_device')          # (an older tree: the routes that exist there)
    K = SAVE_POINTS[-1]

    def free(results):
        for r in results or ():
            r.free()

    def ck(ks, **kw):
        results, trace = sweep.run_tasks_checkpoints_device(tasks, objects, psf_sets, ks, BRIGHT, 'f32', **kw)
        free(results)
        return trace
    routes = {
        'plain': lambda: sweep.run_tasks_device(tasks, objects, psf_sets, K, BRIGHT, 'f32').free(),
        'sweep20': lambda: sweep.run_tasks_device(tasks, objects, psf_sets, 20, BRIGHT, 'f32').free(),
        'curve': lambda: sweep.bias_variance_vs_iterations(objects, psf_sets, seeds, SAVE_POINTS, BRIGHT, 'f32')[1],
    }
    if have_ck:
        routes.update({
            'loop': lambda: sweep._bias_variance_one_sweep_per_k(tasks, keys, objects, psf_sets, SAVE_POINTS, BRIGHT, 'f32', 0, None, None, 0.1),
            'ck7': lambda: ck(SAVE_POINTS),
            'trace7': lambda: ck(SAVE_POINTS, estimates=False),
            'trace_all': lambda: ck(list(range(1, K + 1)), estimates=False),
        })
    if a.only:
        routes = {k: routes[k] for k in a.only.split(',')}
    n_pix = sum(objects[o].shape[-2] * objects[o].shape[-1] for o, _, _ in tasks)
    say('# config 4: %d tasks, %d keys, %.1f MB of f32 estimates per checkpoint; routes %s' % (len(tasks), len(keys), 4 * n_pix / 1e6, ' '.join(routes)))
    first = {name: fn() for name, fn in routes.items()}                # warm-up: plans, buffers
    if 'loop' in first and 'curve' in first:
        say('curve == loop, bit for bit: %s' % np.array_equal(first['loop'], first['curve']))
    if 'trace7' in first and 'ck7' in first:
        say('trace with and without estimates, bit for bit: %s' % np.array_equal(first['trace7'], first['ck7']))
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            t = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t)
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        say('%-9s ms: %s  median %.3f  min %.3f  max %.3f' % (name, ' '.join('%.3f' % (1e3 * x) for x in ts), 1e3 * med[name], 1e3 * min(ts), 1e3 * max(ts)))
    if 'loop' in med and 'curve' in med:
        say('loop / curve (medians) %.3f; sum(K) / max(K) = %.3f' % (med['loop'] / med['curve'], sum(SAVE_POINTS) / K))
    for name, n_ck in (('ck7', 7), ('trace7', 7), ('trace_all', K)):
        if name in med and 'plain' in med:
            say('%s: %.3f ms over plain, %.1f %% of the run, %.1f us per checkpoint of all tasks'
                % (name, 1e3 * (med[name] - med['plain']), 100 * (med[name] - med['plain']) / med[name], 1e6 * (med[name] - med['plain']) / n_ck))
    if a.copy:
        from ensemble_bench import copy_seconds
        from rescan_line_sted_amd._lib import Context
        # a checkpoint with estimates and trace reads est and obj and writes the estimates: 12 bytes per f32 pixel; the copy reads
        # and writes nbytes each
        ts = copy_seconds(Context.get(0), 6 * n_pix, a.repeats)
        say('copy of the bytes of one checkpoint (%.1f MB moved) ms: %s  median %.3f -> %.1f GB/s'
            % (12 * n_pix / 1e6, ' '.join('%.3f' % (1e3 * x) for x in ts), 1e3 * float(np.median(ts)), 12 * n_pix / float(np.median(ts)) / 1e9))


if __name__ == '__main__':
    main()
