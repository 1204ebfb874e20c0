#!/usr/bin/env python3
"""Scoring a sweep's estimates against their true objects: the route through the host against the ring statistics on the device
(manual study).  Two workloads:

  512     64 f32 estimates of 512 x 512 (the astronaut, each pixel repeated four times each way; one point-STED PSF, 64 seeds, 5
          iterations) against one truth
  config4 the 1152 results of BASELINE config 4 at 128 x 128 / 160 x 160 (4 objects x 18 PSF sets x 16 seeds, 20 iterations)

and two routes to the per-ring sum of |fft2(estimate) - fft2(scaled truth)|^2 of every task:

  host    DeviceResults.download() + quality.fourier_error per image + numpy ring binning (np.bincount on a prepared table)
  device  sweep.score_tasks

and, with --sectors S (the angle-resolved statistics, rl_ring_sector_stats), two more:

  sectors sweep.score_tasks(n_sectors=S): ROWS and COLS are the launches of `device`, so the difference is k_ring_reduce_sectors
          against k_ring_reduce plus S times the result bytes
  angles  what the sectors replace: DeviceResults.download() + quality.error_vs_spatial_frequency at the figure's two angles (0 and
          90 / num_angles degrees with num_angles = S / 2) per estimate

warmed, alternated in one process, --repeats times each, a host clock around calls that end in a synchronise.  Prints every time, the
median and the spread, the largest relative difference of the two routes' field 4, and the float64 operations of the two matrix
products from the shapes (8 ny nx (nx + ny) per pair: a complex multiply-add is four fused multiply-adds).

    python tools/gpu/ring_stats_bench.py [--workload 512|config4|both] [--repeats 5] [--sectors 6] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/gpu/ring_stats_bench.py --device-only --repeats 3 [--sectors 6]
    python tools/gpu/ring_stats_bench.py --rates DIR/.../kernel_stats.csv --device-only --repeats 3 [--sectors 6]
      (the achieved FLOP/s of k_ring_rows / k_ring_cols in such a trace: the run's operation count over the kernels' total time)
"""
import argparse
import csv
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BRIGHT = 5e10
# image shapes of the workloads' tasks (config 4: three 128 x 128 objects and the 160 x 160 cat, 18 PSF sets x 16 seeds each)
TASK_SHAPES = {'512': [(512, 512)] * 64, 'config4': [(128, 128)] * 864 + [(160, 160)] * 288}


def ring_table(ny, nx):
    """The ring of every bin (include/rlsted.h), R = min(ny, nx) // 2 for bins outside every ring; Python integers."""
    R = min(ny, nx) // 2
    sy = [k if k <= ny // 2 else k - ny for k in range(ny)]
    sx = [k if k <= nx // 2 else k - nx for k in range(nx)]
    t = np.empty((ny, nx), dtype=np.int64)
    for ky in range(ny):
        for kx in range(nx):
            t[ky, kx] = min(math.isqrt(4 * R * R * ((sy[ky] * nx) ** 2 + (sx[kx] * ny) ** 2)) // (ny * nx), R)
    return t


def workload(name):
    from rescan_line_sted_amd import psf
    objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
    if name == '512':
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g8_fig2_psfs.npz'))
        objects = {'astronaut512': np.kron(objs['astronaut'][0].astype(np.float64), np.ones((4, 4)))}
        return objects, {'point': list(g['1p5x_lr/point_sted_psf'])}, range(64), 5
    objects = {n: objs[n][0].astype(np.float64) for n in ('astronaut', 'cat', 'lines', 'rings')}
    doses = ('1p0x', '1p5x', '2p0x', '2p5x', '3p0x', '4p0x')
    sets, _ = psf.figure_2_psfs([d + s for d in doses for s in ('_ld', '_lr')])
    psf_sets = {}
    for d in doses:
        psf_sets[d + '_point'] = [np.asarray(p) for p in sets[d + '_lr_point_sted']]
        for s in ('_ld', '_lr'):
            psf_sets[d + s] = [np.asarray(p) for p in sets[[k for k in sets if k.startswith(d + s + '_line_')][0]]]
    return objects, psf_sets, range(16), 20


def product_flops(shapes):
    return sum(8 * ny * nx * (nx + ny) for ny, nx in shapes)


def host_route(res, tasks, objects, tables):
    from rescan_line_sted_amd import quality
    est = res.download()
    out = []
    for (o, _, _), e in zip(tasks, est):
        obj = objects[o]
        fe = np.fft.ifftshift(quality.fourier_error(e, (BRIGHT / obj.sum()) * obj)) * e.size
        t = tables[e.shape]
        out.append(np.bincount(t.ravel(), weights=(fe * fe).ravel(), minlength=min(e.shape) // 2 + 1)[:min(e.shape) // 2])
    return out


def device_route(res, tasks, objects, sectors=None):
    from rescan_line_sted_amd import sweep
    return sweep.score_tasks(res, tasks, objects, BRIGHT, n_sectors=sectors)


def angles_route(res, tasks, objects, sectors):
    from rescan_line_sted_amd import quality
    est = res.download()
    worst = 90.0 / max(sectors // 2, 1)
    return [[quality.error_vs_spatial_frequency(e, (BRIGHT / objects[o].sum()) * objects[o], ang) for ang in (0.0, worst)]
            for (o, _, _), e in zip(tasks, est)]


def scorings(repeats, sectors):
    """score_tasks calls of one workload's run: the warm-up and `repeats`, of each device route."""
    return (repeats + 1) * (2 if sectors else 1)


def run(name, repeats, device_only, say, sectors=None):
    from rescan_line_sted_amd import sweep
    objects, psf_sets, seeds, iterations = workload(name)
    tasks = sweep.make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    res = sweep.run_tasks_device(tasks, objects, psf_sets, iterations, BRIGHT, 'f32')
    shapes = [tuple(s) for s in res.shapes]
    flops = product_flops(shapes)
    assert sorted(shapes) == sorted(TASK_SHAPES[name])
    say('# workload %s: %d tasks, shapes %s, %.3f GFLOP in the two products per scoring (8 ny nx (nx + ny) per pair), %.1f MB of estimates'
        % (name, len(tasks), sorted(set(shapes)), flops / 1e9, res.n * res.itemsize / 1e6))
    tables = {s: ring_table(*s) for s in set(shapes)}
    dev = device_route(res, tasks, objects)                        # warm-up of both routes (--rates counts this call too)
    times = {'host': [], 'device': [], 'sectors': [], 'angles': []}
    if sectors:
        cells = device_route(res, tasks, objects, sectors)
        worst = max(float(np.max(np.abs(np.asarray(c).sum(axis=1)[:, 4] - np.asarray(d)[:, 4]) / np.asarray(d)[:, 4])) for c, d in zip(cells, dev))
        say('%s: largest relative difference of field 4 between the sectors summed and the rings %.3g' % (name, worst))
        if not device_only:
            angles_route(res, tasks[:8], objects, sectors)
    if not device_only:
        host = host_route(res, tasks, objects, tables)
        worst = max(float(np.max(np.abs(np.asarray(d)[:, 4] - h) / np.maximum(np.abs(h), 1e-300))) for d, h in zip(dev, host))
        say('%s: largest relative difference of field 4 between the routes %.3g' % (name, worst))
    for _ in range(repeats):
        if not device_only:
            t = time.perf_counter()
            host_route(res, tasks, objects, tables)
            times['host'].append(time.perf_counter() - t)
        t = time.perf_counter()
        device_route(res, tasks, objects)
        times['device'].append(time.perf_counter() - t)
        if sectors:
            t = time.perf_counter()
            device_route(res, tasks, objects, sectors)
            times['sectors'].append(time.perf_counter() - t)
            if not device_only:
                t = time.perf_counter()
                angles_route(res, tasks, objects, sectors)
                times['angles'].append(time.perf_counter() - t)
    for route in ('host', 'device', 'sectors', 'angles'):
        ts = times[route]
        if ts:
            say('%s %-7s ms: %s  median %.2f  min %.2f  max %.2f' % (name, route, ' '.join('%.2f' % (1e3 * x) for x in ts),
                                                                     1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts)))
    if times['host']:
        say('%s: host / device (medians) %.1f' % (name, float(np.median(times['host'])) / float(np.median(times['device']))))
    if times['sectors']:
        say('%s: sectors / device (medians) %.2f' % (name, float(np.median(times['sectors'])) / float(np.median(times['device']))))
    if times['angles']:
        say('%s: angles / sectors (medians) %.1f' % (name, float(np.median(times['angles'])) / float(np.median(times['sectors']))))
    res.free()


def rates(path, flops, say):
    rows = [r for r in csv.DictReader(open(path)) if 'k_ring_' in r['Name']]
    for r in rows:
        say('%s: %s calls, %.3f ms in all, %.1f us on average' % (r['Name'], r['Calls'], int(r['TotalDurationNs']) / 1e6, float(r['AverageNs']) / 1e3))
    ns = sum(int(r['TotalDurationNs']) for r in rows if 'k_ring_rows' in r['Name'] or 'k_ring_cols' in r['Name'])
    if not ns:
        raise SystemExit('no k_ring_rows / k_ring_cols in %s' % path)
    say('products: %.3f GFLOP over %.3f ms of k_ring_rows + k_ring_cols = %.2f TFLOP/s float64' % (flops / 1e9, ns / 1e6, flops / ns / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='both', choices=('512', 'config4', 'both'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--sectors', type=int, default=0, help='also time score_tasks(n_sectors=S) and the two-angle host route')
    ap.add_argument('--rates', default=None, help='kernel_stats.csv of a rocprofv3 trace of the same command line')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    log = open(a.out, 'a') if a.out else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()
    names = ('512', 'config4') if a.workload == 'both' else (a.workload,)
    if a.rates:                                                    # no device work: the operation count of that command line
        rates(a.rates, sum(product_flops(TASK_SHAPES[n]) for n in names) * scorings(a.repeats, a.sectors), say)
        return
    for n in names:
        run(n, a.repeats, a.device_only, say, a.sectors or None)


if __name__ == '__main__':
    main()
