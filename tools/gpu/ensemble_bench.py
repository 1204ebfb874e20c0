#!/usr/bin/env python3
"""Reducing a sweep's seeds to ensemble statistics: the route through the host against rl_ensemble_stats on the device (manual
study).  Two workloads, those of tools/gpu/ring_stats_bench.py:

  512     64 f32 estimates of 512 x 512 -- 4 groups of 16
  config4 the 1152 results of BASELINE config 4 at 128 x 128 / 160 x 160 -- 72 (object, PSF set) keys of 16 seeds

and these routes to every key's per-pixel mean and variance maps and the six pixel sums:

  maps     sweep.ensemble_tasks(maps=True)   (the truths' upload, the map buffers' allocation, one call per shape)
  scalars  sweep.ensemble_tasks(maps=False)
  call     the rl_ensemble_stats calls alone, on truths and map buffers that are already there -- what the traffic is counted for
  copy     a device-to-device hipMemcpy that reads half and writes half of the bytes `call` must move
  host     what the device route replaces: DeviceResults.download() + numpy float64 per key

warmed, alternated in one process, --repeats times each, a host clock around calls that end in a synchronise.  The bytes `call`
must move, per group of n members of N pixels of T: 2 n N sizeof(T) in (two passes over the members) + 8 N (the float64 truth),
16 N out (the two maps).  Prints every time, the medians, bytes / second of `call` and of `copy` and their ratio, and the largest
relative difference of the two routes' sums.

    python tools/gpu/ensemble_bench.py [--workload 512|config4|both] [--repeats 5] [--device-only] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ring_stats_bench import BRIGHT, workload          # noqa: E402  (the same two workloads)


def host_route(res, tasks, objects):
    from rescan_line_sted_amd import sweep
    est = res.download()
    keys, members = sweep.ensemble_keys(tasks)
    out = np.zeros((len(keys), 6))
    maps = []
    for k, ((o, _), mem) in enumerate(zip(keys, members)):
        x = np.stack([est[i] for i in mem])
        st = (BRIGHT / objects[o].sum()) * objects[o]
        mean = x.mean(axis=0)
        var = x.var(axis=0, ddof=1) if len(mem) > 1 else np.zeros_like(mean)
        out[k] = [len(mem), mean.sum(), var.sum(), ((mean - st) ** 2).sum(), ((x - st) ** 2).mean(axis=0).sum(), (st * st).sum()]
        maps.append((mean, var))
    return out, maps


class Prepared:
    """Truths and map buffers kept on the device: the rl_ensemble_stats calls of ensemble_tasks without what surrounds them."""

    def __init__(self, res, tasks, objects):
        from rescan_line_sted_amd import sweep
        self.res = res
        self.keys, self.members = sweep.ensemble_keys(tasks)
        self.truths, where, scales = sweep._upload_truths(tasks, objects, BRIGHT, res.ctx.device)
        shapes = [res.shapes[m[0]] for m in self.members]
        self.by_shape = sweep._by_shape(shapes)
        order = [k for ks in self.by_shape.values() for k in ks]
        self.means = sweep.DeviceResults.with_layout(shapes, order, 'f64', res.ctx.device)
        self.variances = sweep.DeviceResults.with_layout(shapes, order, 'f64', res.ctx.device)
        self.t_idx = [where[o] for o, _ in self.keys]
        self.scale = [scales[o] for o, _ in self.keys]
        self.bytes = sum((2 * len(m) * res.itemsize + 8 + 16) * s[0] * s[1] for m, s in zip(self.members, shapes))

    def call(self):
        out = np.zeros((len(self.keys), 6))
        for ks in self.by_shape.values():
            out[ks] = self.res._ensemble_into([self.members[k] for k in ks], self.truths, [self.t_idx[k] for k in ks],
                                              [self.scale[k] for k in ks], self.means.address(ks[0]), self.variances.address(ks[0]))
        return out

    def free(self):
        for b in (self.truths, self.means, self.variances):
            b.free()


def copy_seconds(ctx, nbytes, repeats):
    """Seconds of a device-to-device hipMemcpy of `nbytes` bytes (read nbytes, write nbytes) between two rl_device_alloc buffers,
    each of `repeats` after a warm-up.  The HIP runtime is the one librlsted.so runs on, called through ctypes."""
    import ctypes
    from rescan_line_sted_amd import _build
    from rescan_line_sted_amd._lib import check, lib
    path = os.path.join(os.path.dirname(os.path.dirname(_build.HIPCC)), 'lib', 'libamdhip64.so')
    hip = ctypes.CDLL(path if os.path.exists(path) else 'libamdhip64.so')
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.rl_device_alloc(ctx.handle, nbytes, ctypes.byref(a)))
    check(lib.rl_device_alloc(ctx.handle, nbytes, ctypes.byref(b)))
    out = []
    try:
        assert hip.hipMemset(a, 1, nbytes) == 0
        for k in range(repeats + 1):
            assert hip.hipDeviceSynchronize() == 0
            t = time.perf_counter()
            assert hip.hipMemcpy(b, a, nbytes, 3) == 0             # hipMemcpyDeviceToDevice
            assert hip.hipDeviceSynchronize() == 0
            if k:
                out.append(time.perf_counter() - t)
    finally:
        lib.rl_device_free(ctx.handle, a)
        lib.rl_device_free(ctx.handle, b)
    return out


def run(name, repeats, device_only, say):
    from rescan_line_sted_amd import sweep
    objects, psf_sets, seeds, iterations = workload(name)
    if name == '512':
        objects = {'astronaut512_%d' % k: v for k in range(4) for v in objects.values()}      # 4 keys of 16 seeds
        seeds = range(16)
    tasks = sweep.make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    res = sweep.run_tasks_device(tasks, objects, psf_sets, iterations, BRIGHT, 'f32')
    prep = Prepared(res, tasks, objects)
    say('# workload %s: %d tasks in %d keys, shapes %s, %.1f MB of estimates, %.1f MB to move per reduction'
        % (name, len(tasks), len(prep.keys), sorted(set(map(tuple, res.shapes))), res.n * res.itemsize / 1e6, prep.bytes / 1e6))
    dev = prep.call()                                             # warm-up of every route
    for maps in (True, False):
        _, _, m, v, sc = sweep.ensemble_tasks(res, tasks, objects, BRIGHT, maps=maps)
        assert np.array_equal(sc, dev)
        if maps:
            m.free()
            v.free()
    if not device_only:
        host, _ = host_route(res, tasks, objects)
        say('%s: largest relative difference of the sums between the routes %.3g'
            % (name, float(np.max(np.abs(dev[:, 1:] - host[:, 1:]) / np.maximum(np.abs(host[:, 1:]), 1e-300)))))
    times = {'maps': [], 'scalars': [], 'call': [], 'host': []}
    for _ in range(repeats):
        for route, maps in (('maps', True), ('scalars', False)):
            t = time.perf_counter()
            _, _, m, v, _ = sweep.ensemble_tasks(res, tasks, objects, BRIGHT, maps=maps)
            times[route].append(time.perf_counter() - t)
            if maps:
                m.free()
                v.free()
        t = time.perf_counter()
        prep.call()
        times['call'].append(time.perf_counter() - t)
        if not device_only:
            t = time.perf_counter()
            host_route(res, tasks, objects)
            times['host'].append(time.perf_counter() - t)
    times['copy'] = copy_seconds(res.ctx, prep.bytes // 2, repeats)
    for route in ('maps', 'scalars', 'call', 'copy', 'host'):
        ts = times[route]
        if ts:
            say('%s %-7s ms: %s  median %.3f  min %.3f  max %.3f' % (name, route, ' '.join('%.3f' % (1e3 * x) for x in ts),
                                                                     1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts)))
    call, copy = float(np.median(times['call'])), float(np.median(times['copy']))
    say('%s: call %.1f GB/s, copy %.1f GB/s (both: %.1f MB over the median), call / copy rate %.2f'
        % (name, prep.bytes / call / 1e9, prep.bytes / copy / 1e9, prep.bytes / 1e6, copy / call))
    if times['host']:
        say('%s: host / maps (medians) %.1f' % (name, float(np.median(times['host'])) / float(np.median(times['maps']))))
    prep.free()
    res.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='both', choices=('512', 'config4', 'both'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    log = open(a.out, 'a') if a.out else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()
    for n in (('512', 'config4') if a.workload == 'both' else (a.workload,)):
        run(n, a.repeats, a.device_only, say)


if __name__ == '__main__':
    main()
