#!/usr/bin/env python3
"""Host-inclusive throughput of Richardson-Lucy on an acquired stack (manual tool; INTEGRATION.md section 5h, DESIGN.md section 4j,
README status table).  512 x 512, 1 view (the 2.0x point-STED PSF), K = 20, 1024 uint16 frames, batch 256, f32 plans.

  deconvolve            the float64 path: set_measurement (2 MB per frame up), iterate, estimate(out=...) (2 MB down), chunk after
                        chunk on one plan, nothing overlapped -- what a caller with measured data had before deconvolve_stack
  stack u16 -> f32      deconvolve_stack: 0.5 MB up, 1 MB down per frame, upload / iterations / download overlapped
  stack u16 -> u16      0.5 MB up, 0.5 MB down

each with ordinary numpy arrays and with page-locked ones (_lib.pinned_empty), warmed once, the median of --repeats runs.  For the
stack the rate is frames / the wall time of rl_stack_run (its times_ms, recorded whole: wall, summed upload, compute and download
event times) -- the plan and the pipeline's blocks exist before, as the plan does for deconvolve; the whole deconvolve_stack call,
set-up included, is recorded beside it.  The two kernels are timed alone between synchronisations (calls, launch overhead inside)
beside an rl_device_copy that moves as many bytes (a copy of n bytes reads n and writes n).

    python tools/gpu/stack_throughput.py [--repeats 3] [--frames 1024] [--out profiles/stack/throughput.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K, N, B = 20, 512, 256
DARK, GAIN = 100.0, 0.46


def frames_u16(F):
    """64 distinct Poisson frames of the 512 x 512 astronaut (a few hundred counts over a dark level of 100), repeated."""
    objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
    obj = np.kron(objs['astronaut'].astype(np.float64), np.ones((1, 4, 4)))[0]
    obj = 40.0 + obj * (900.0 / obj.max())
    rng = np.random.default_rng(7)
    base = (DARK + rng.poisson(obj / GAIN, size=(min(F, 64), N, N))).astype(np.uint16)
    return np.ascontiguousarray(np.tile(base, (-(-F // len(base)), 1, 1))[:F])


def median(v):
    return float(np.median(v))


def float64_path(_lib, psf, meas, out, repeats):
    plan = _lib.DeconvPlan(psf, B, N, N, dtype='f32')
    F = len(meas)
    wall, device = [], []
    for rep in range(repeats + 1):
        t0, dev_ms = time.perf_counter(), 0.0
        for f in range(0, F, B):
            plan.set_measurement(meas[f:f + B])
            plan.reset_estimate()
            plan.iterate(K)
            dev_ms += plan.last_ms()['iterate_ms']
            plan.estimate(out=out[f:f + B])
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
            device.append(dev_ms)
    return {'wall_ms': median(wall), 'iterate_ms_events': median(device), 'frames_per_s': F / median(wall) * 1e3,
            'bytes_per_frame': N * N * 16}


def stack_path(stack, psf, raw, out, out_dtype, repeats):
    cam = stack.CameraModel(dark=DARK, gain=GAIN, saturation=65535)
    F = len(raw)
    runs, calls = [], []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        _, info = stack.deconvolve_stack(raw, psf, K, camera=cam, dtype='f32', out_dtype=out_dtype, batch=B, out=out)
        if rep:
            calls.append((time.perf_counter() - t0) * 1e3)
            runs.append(info['times'])
    times = {k: median([r[k] for r in runs]) for k in runs[0]}
    return {'times_ms': times, 'call_ms_with_setup': median(calls), 'frames_per_s': F / times['wall_ms'] * 1e3,
            'frames_per_s_with_setup': F / median(calls) * 1e3, 'bytes_per_frame': N * N * (2 + out.itemsize), 'chunks': info['chunks'],
            'saturated': int(info['saturated'].sum()), 'clipped': int(info['clipped'].sum()), 'clamped': int(info['clamped'].sum())}


def kernels_alone(_lib, repeats):
    """rl_ingest u16 -> f32 and rl_export f32 -> f32 / u16 on 256 frames, each beside a device copy of as many bytes."""
    L, ctx = _lib.lib, _lib.Context.get(0)
    n = B * N * N

    def alloc(nbytes):
        p = ctypes.c_void_p()
        _lib.check(L.rl_device_alloc(ctx.handle, nbytes, ctypes.byref(p)))
        return p
    raw, f32, out, spare = alloc(2 * n), alloc(4 * n), alloc(4 * n), alloc(4 * n)
    stats = alloc(B * 4 * 8)
    ones = np.ones(n // 4)                                        # (n u16 values of 0x3ff0 / 0: any bytes will do)
    _lib.check(L.rl_device_upload(ctx.handle, raw, _lib.RL_F64, ones.size, _lib.ptr(ones)))

    def timed(fn):
        best = []
        for rep in range(repeats + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn())
            ctx.synchronize()
            if rep:
                best.append((time.perf_counter() - t0) * 1e3)
        return median(best)
    rows = {}
    for name, moved, fn in (
            ('ingest_u16_f32', 6 * n, lambda: L.rl_ingest(ctx.handle, raw, 1, B, N, N, 0, 0, 1, 1, B, B, 1, N, N, None, DARK, GAIN, 1e-9, 65535.0, f32, 0, stats)),
            ('export_f32_f32', 8 * n, lambda: L.rl_export(ctx.handle, f32, 0, B, N, N, 1.0, out, 0, stats)),
            ('export_f32_u16', 6 * n, lambda: L.rl_export(ctx.handle, f32, 0, B, N, N, 1.0, out, 2, stats))):
        ms = timed(fn)
        copy_ms = timed(lambda: L.rl_device_copy(ctx.handle, spare, f32, moved // 2))
        rows[name] = {'ms': ms, 'bytes_moved': moved, 'gb_per_s': moved / ms / 1e6, 'copy_of_as_many_bytes_ms': copy_ms, 'over_copy': ms / copy_ms}
    for p in (raw, f32, out, spare, stats):
        L.rl_device_free(ctx.handle, p)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stack', 'throughput.json'))
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib, stack
    import bench
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    psf = bench.workload(N)[1]
    F = args.frames
    raw = frames_u16(F)
    res = {'image': [N, N], 'views': 1, 'iterations': K, 'frames': F, 'batch': B, 'dtype': 'f32', 'repeats': args.repeats, 'paths': {}}
    # the float64 path's measurement: what a caller forms on the host today
    meas = (np.maximum((raw.astype(np.float64) - DARK) * GAIN, 0.0) + 1e-9)[:, None]
    for memory in ('pageable', 'page-locked'):
        pin = memory == 'page-locked'
        m, o = (_lib.pinned_empty(meas.shape), _lib.pinned_empty((F, N, N))) if pin else (meas, np.empty((F, N, N)))
        if pin:
            m[:] = meas
        res['paths']['deconvolve float64 / ' + memory] = float64_path(_lib, psf, m, o, args.repeats)
        del m, o
    del meas
    for out_dtype, np_out in (('f32', np.float32), ('u16', np.uint16)):
        for memory in ('pageable', 'page-locked'):
            pin = memory == 'page-locked'
            r, o = (_lib.pinned_empty(raw.shape, np.uint16), _lib.pinned_empty((F, N, N), np_out)) if pin else (raw, np.empty((F, N, N), dtype=np_out))
            if pin:
                r[:] = raw
            res['paths']['stack u16 -> %s / %s' % (out_dtype, memory)] = stack_path(stack, psf, r, o, out_dtype, args.repeats)
            del r, o
    res['kernels'] = kernels_alone(_lib, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    for name, row in res['paths'].items():
        print('%-36s %8.0f frames/s  %s' % (name, row['frames_per_s'], json.dumps(row['times_ms'] if 'times_ms' in row else {'wall_ms': row['wall_ms']})))
    print(json.dumps(res['kernels']))


if __name__ == '__main__':
    main()
