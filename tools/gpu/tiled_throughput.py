#!/usr/bin/env python3
"""Throughput of tiled Richardson-Lucy (manual tool; DESIGN.md section 4i, README status table).  Two workloads, f32, K = 20, the
2.0x figure-2 PSFs (107 x 107), default tile, margin and overlap:

  8192x1   one 8192 x 8192 image, 1 view  (the point-STED PSF)
  4096x4   one 4096 x 4096 image, 4 views (the line-STED PSFs)

The steps of tiling.deconvolve_tiled are run one by one on a measurement that is already on the device, each between two
synchronisations of the context under a host clock (the Richardson-Lucy part also by the plan's own HIP events,
DeconvPlan.last_ms), warmed once, --repeats times.  Reported per workload:

  total_ms, gpixel_per_s     gather + iterate + copies + blend of the whole image; image pixels / total
  share_moving               (gather + copies + blend) / total
  gather, blend              their time and bytes written per second, beside rl_device_copy calls of as many bytes (the yardstick:
                             one copy per chunk for the gather, one for the blend), timed the same way.  These are times of CALLS:
                             the staging of the slot list or the tables and the synchronisation are inside.  The kernels alone come
                             from a kernel trace of this tool in a run of its own
  whole_image (4096x4 only)  the same measurement through deconvolve on one whole-image plan at the same K

    python tools/gpu/tiled_throughput.py [--repeats 3] [--workload 8192x1|4096x4|both] [--out profiles/tiled/throughput.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K = 20
WORKLOADS = {'8192x1': (8192, '2p0x_lr/point_sted_psf'), '4096x4': (4096, '2p0x_lr/line_sted_psfs')}


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(name, repeats):
    from rescan_line_sted_amd import _lib, tiling
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    n, key = WORKLOADS[name]
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g8_fig2_psfs.npz'))
    psfs = [np.asarray(p, dtype=np.float64) for p in g[key]]
    V = len(psfs)
    rng = np.random.default_rng(n)
    meas = (rng.poisson(100.0, size=(1, V, n, n)) + 1e-9).astype(np.float64)
    margin = tiling.DEFAULT_MARGIN
    layout = tiling.TileLayout((n, n), tiling.default_tile(psfs), tiling.default_overlap(margin), margin)
    slots = layout.slots(1)
    tiles, batch = len(slots), min(len(slots), 32)
    ty, tx = layout.tile_shape
    dev = tiling._Device(psfs, batch, (ty, tx), 'f32', 0, None, None, 0.1)
    rows = []
    try:
        dev.upload(meas)
        store, out = dev.alloc(tiles * ty * tx), dev.alloc(n * n)
        spare = dev.alloc(max(batch * V * ty * tx, n * n))
        gather_bytes, blend_bytes = batch * V * ty * tx * 4, n * n * 4
        for rep in range(repeats + 1):                      # (the first pass warms every kernel and is dropped)
            t = {'gather': 0.0, 'iterate': 0.0, 'iterate_events': 0.0, 'copy': 0.0, 'gather_yardstick': 0.0}
            for first in range(0, tiles, batch):
                m = min(batch, tiles - first)
                chunk = np.full((batch, 3), (-1, 0, 0), dtype=np.intc)
                chunk[:m] = slots[first:first + m]
                t['gather'] += timed(dev.ctx, lambda: dev.gather(chunk))
                t['iterate'] += timed(dev.ctx, lambda: dev.iterate(K, None))
                t['iterate_events'] += dev.plan.last_ms()['iterate_ms']
                t['copy'] += timed(dev.ctx, lambda: dev.store(store, first, m))
                t['gather_yardstick'] += timed(dev.ctx, lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, spare, dev.meas, gather_bytes)))
            t['blend'] = timed(dev.ctx, lambda: dev.blend(store, layout, 1, out))
            t['blend_yardstick'] = timed(dev.ctx, lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, spare, out, blend_bytes)))
            if rep:
                rows.append(t)
    finally:
        dev.close()
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    total = med['gather'] + med['iterate'] + med['copy'] + med['blend']
    chunks = (tiles + batch - 1) // batch
    res = {'workload': name, 'image': [n, n], 'views': V, 'iterations': K, 'dtype': 'f32', 'tile': [ty, tx], 'margin': margin,
           'overlap': tiling.default_overlap(margin), 'tiles': tiles, 'batch': batch, 'chunks': chunks, 'repeats': repeats, 'ms': med,
           'total_ms': total, 'gpixel_per_s': n * n / total / 1e6, 'share_moving': (med['gather'] + med['copy'] + med['blend']) / total,
           'gather_gb_per_s_written': chunks * gather_bytes / med['gather'] / 1e6,
           'gather_over_copy': med['gather'] / med['gather_yardstick'],
           'blend_gb_per_s_written': blend_bytes / med['blend'] / 1e6, 'blend_over_copy': med['blend'] / med['blend_yardstick']}
    if name == '4096x4':
        plan = _lib.DeconvPlan(psfs, 1, n, n, dtype='f32')
        whole = []
        for rep in range(repeats + 1):
            t0 = time.perf_counter()
            deconvolve(meas, psfs, K, dtype='f32', plan=plan)
            host_ms = (time.perf_counter() - t0) * 1e3
            if rep:
                whole.append((plan.last_ms()['iterate_ms'], host_ms))
        it = float(np.median([w[0] for w in whole]))
        res['whole_image'] = {'iterate_ms_events': it, 'call_ms_with_transfers': float(np.median([w[1] for w in whole])),
                              'gpixel_per_s': n * n / it / 1e6, 'tiled_iterate_ms_events': med['iterate_events'],
                              'tiled_total_over_whole_iterate': total / it}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--workload', default='both', choices=['both'] + sorted(WORKLOADS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tiled', 'throughput.json'))
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    results = [run(w, args.repeats) for w in (sorted(WORKLOADS) if args.workload == 'both' else [args.workload])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'results': results}, f, indent=1)
        f.write('\n')
    for r in results:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
