#!/usr/bin/env python3
"""Throughput of the camera calibration (manual tool; INTEGRATION.md section 5k, DESIGN.md section 4m, README status table).

  accumulate       rl_calib_accumulate alone, between synchronisations (the call and its launch overhead inside), on 256 frames of
                   2048 x 2048 uint16 (2048 workgroups, no frame split) and on 4096 frames of 512 x 512 uint16 (128 workgroups x 8
                   parts of the frame split, combined with 64-bit integer atomics), each beside an rl_device_copy of the bytes it
                   reads (a copy of n bytes reads n and writes n) -- the project's figure for streaming kernels
  temporal_stats   end to end on the 2048 x 2048 stack from pageable host memory: upload and kernel time apart
  numpy            the same mean and variance on the host (float64 temporaries), on --numpy-frames of those frames
  repair           rl_repair_pixels at 0.1 % defects on 256 images of 512 x 512, f32
  stack lines      the two page-locked deconvolve_stack lines of tools/gpu/stack_throughput.py (u16 -> f32, u16 -> u16; camera without
                   defects), to be taken on the parent commit and on this one in the same session, alternating:
                   --stack-lines-only FILE writes just those; --parent-stack-lines / --this-stack-lines FILES merge such runs
                   into this run's record

each warmed once, the median of --repeats runs.

    python tools/gpu/calibration_throughput.py [--repeats 3] [--out profiles/calibration/throughput.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def median(v):
    return float(np.median(v))


def timed(ctx, check, fn, repeats):
    runs = []
    for rep in range(repeats + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        check(fn())
        ctx.synchronize()
        if rep:
            runs.append((time.perf_counter() - t0) * 1e3)
    return median(runs), runs


def accumulate_alone(_lib, n, frames, repeats):
    """rl_calib_accumulate of `frames` frames of n x n uint16 that lie on the device, beside a copy of as many bytes."""
    L, ctx = _lib.lib, _lib.Context.get(0)
    nbytes = frames * n * n * 2
    raw, spare = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.rl_device_alloc(ctx.handle, nbytes, ctypes.byref(raw)))
    _lib.check(L.rl_device_alloc(ctx.handle, nbytes, ctypes.byref(spare)))
    chunk = np.random.default_rng(1).integers(90, 4000, min(nbytes // 2, 1 << 24)).astype(np.uint16)
    for at in range(0, nbytes, chunk.nbytes):
        m = min(chunk.nbytes, nbytes - at)
        _lib.check(L.rl_device_upload_bytes(ctx.handle, ctypes.c_void_p(raw.value + at), chunk.ctypes.data_as(ctypes.c_void_p), m))
    h = ctypes.c_void_p()
    _lib.check(L.rl_calib_create(ctx.handle, 1, n, n, 0, 0, n, n, ctypes.byref(h)))

    def run():
        rc = L.rl_calib_reset(h)
        return rc or L.rl_calib_accumulate(h, raw, frames)
    ms, runs = timed(ctx, _lib.check, run, repeats)
    reset_ms, _ = timed(ctx, _lib.check, lambda: L.rl_calib_reset(h), repeats)
    copy_ms, copy_runs = timed(ctx, _lib.check, lambda: L.rl_device_copy(ctx.handle, spare, raw, nbytes), repeats)
    L.rl_calib_destroy(h)
    for p in (raw, spare):
        L.rl_device_free(ctx.handle, p)
    ms -= reset_ms                                                # (the reset zeroes 16 bytes per pixel between the runs)
    return {'window': [n, n], 'frames': frames, 'bytes_read': nbytes, 'ms': ms, 'runs_ms_with_reset': runs, 'reset_ms': reset_ms,
            'gb_per_s': nbytes / ms / 1e6, 'copy_of_the_bytes_ms': copy_ms, 'copy_runs_ms': copy_runs, 'over_copy': ms / copy_ms}


def end_to_end(calibration, raw, repeats):
    rows = []
    for rep in range(repeats + 1):
        mean, var, info = calibration.temporal_stats(raw)
        if rep:
            rows.append(info['times'])
    times = {k: median([r[k] for r in rows]) for k in rows[0]}
    return {'frames': int(raw.shape[0]), 'sensor': list(raw.shape[1:]), 'bytes': int(raw.nbytes), 'chunks': info['chunks'], 'times_ms': times,
            'upload_gb_per_s': raw.nbytes / times['upload_ms'] / 1e6, 'gb_per_s': raw.nbytes / times['wall_ms'] / 1e6}, mean, var


def numpy_stats(raw):
    t0 = time.perf_counter()
    x = raw.astype(np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0, ddof=1)
    return (time.perf_counter() - t0) * 1e3, mean, var


def repair_alone(_lib, repeats):
    L, ctx = _lib.lib, _lib.Context.get(0)
    n, ny, nx = 256, 512, 512
    rng = np.random.default_rng(2)
    mask = (rng.random((ny, nx)) < 0.001).astype(np.uint8)
    img = ctypes.c_void_p()
    _lib.check(L.rl_device_alloc(ctx.handle, n * ny * nx * 4, ctypes.byref(img)))
    one = rng.random((ny, nx)).astype(np.float32)
    for i in range(n):
        _lib.check(L.rl_device_upload_bytes(ctx.handle, ctypes.c_void_p(img.value + i * one.nbytes), one.ctypes.data_as(ctypes.c_void_p), one.nbytes))
    ms, runs = timed(ctx, _lib.check, lambda: L.rl_repair_pixels(ctx.handle, img, 0, n, ny, nx, mask.ctypes.data_as(ctypes.c_void_p), 3, None), repeats)
    L.rl_device_free(ctx.handle, img)
    return {'images': n, 'shape': [ny, nx], 'dtype': 'f32', 'defects': int(mask.sum()), 'radius': 3, 'ms': ms, 'runs_ms': runs,
            'note': 'the call: the host builds and uploads the list, one launch over images x defects'}


def stack_lines(repeats):
    """The two page-locked deconvolve_stack lines of stack_throughput.py, its own code and workload."""
    import bench
    import stack_throughput as st
    from rescan_line_sted_amd import _lib, stack
    psf = bench.workload(st.N)[1]
    raw = st.frames_u16(1024)
    rows = {}
    for out_dtype, np_out in (('f32', np.float32), ('u16', np.uint16)):
        r, o = _lib.pinned_empty(raw.shape, np.uint16), _lib.pinned_empty((1024, st.N, st.N), np_out)
        r[:] = raw
        row = st.stack_path(stack, psf, r, o, out_dtype, repeats)
        rows['stack u16 -> %s / page-locked' % out_dtype] = {'frames_per_s': row['frames_per_s'], 'times_ms': row['times_ms']}
        del r, o
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--numpy-frames', type=int, default=64)
    ap.add_argument('--stack-lines-only', default=None)
    ap.add_argument('--parent-stack-lines', nargs='*', default=[])
    ap.add_argument('--this-stack-lines', nargs='*', default=[])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'calibration', 'throughput.json'))
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    if args.stack_lines_only:
        rows = stack_lines(args.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(args.stack_lines_only)), exist_ok=True)
        with open(args.stack_lines_only, 'w') as f:
            json.dump(rows, f, indent=1)
        print(json.dumps(rows))
        return
    from rescan_line_sted_amd import calibration
    res = {'repeats': args.repeats, 'accumulate': {}}
    res['accumulate']['2048x2048 x 256'] = accumulate_alone(_lib, 2048, 256, args.repeats)
    res['accumulate']['512x512 x 4096 (frame split)'] = accumulate_alone(_lib, 512, 4096, args.repeats)
    rng = np.random.default_rng(3)
    base = (100 + rng.poisson(300.0, (16, 2048, 2048))).astype(np.uint16)
    raw = np.ascontiguousarray(np.tile(base, (16, 1, 1)))                # 256 frames, 2 GiB
    res['temporal_stats'], mean, var = end_to_end(calibration, raw, args.repeats)
    sub = raw[:args.numpy_frames]
    np_ms, np_mean, np_var = numpy_stats(sub)
    d_mean, d_var, _ = calibration.temporal_stats(sub)
    res['numpy'] = {'frames': int(sub.shape[0]), 'ms': np_ms, 'ms_scaled_to_256_frames': np_ms * 256 / sub.shape[0],
                    'largest_difference_of_the_means': float(np.abs(np_mean - d_mean).max()),
                    'largest_relative_difference_of_the_variances': float((np.abs(np_var - d_var) / np.maximum(d_var, 1e-300)).max())}
    res['repair'] = repair_alone(_lib, args.repeats)
    def load(paths):
        rows = []
        for path in paths:
            with open(path) as f:
                rows.append(json.load(f))
        return rows
    # (each entry a median of --repeats runs; the files: --stack-lines-only runs of the same session, the two trees alternating)
    res['stack_lines'] = {'this': load(args.this_stack_lines) + [stack_lines(args.repeats)], 'parent': load(args.parent_stack_lines)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'accumulate'}))
    for name, row in res['accumulate'].items():
        print('%-32s %8.3f ms  %7.1f GB/s  copy %8.3f ms  %.2fx' % (name, row['ms'], row['gb_per_s'], row['copy_of_the_bytes_ms'], row['over_copy']))


if __name__ == '__main__':
    main()
