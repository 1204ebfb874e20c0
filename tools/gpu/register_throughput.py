#!/usr/bin/env python3
"""Throughput of the registration path (manual tool; INTEGRATION.md section 5i, DESIGN.md section 4k, README status table).

  sums          rl_register_sums at 512 x 512, R in {4, 8, 16}, M = R, 256 pairs (one reference, 256 moving images), f32: the time of
                the whole call (launches, the second-stage reduction, the download of the sums; it ends in a synchronise), the
                achieved fused multiply-adds per second against 2 (2 R + 1)^2 (ny - 2 M)(nx - 2 M) per pair (S_bb and S_ab; the S_b
                additions are not counted), and the bytes the call has to move (the images once, the partial sums written and read)
  shift         rl_shift_images on 256 images of 512 x 512, f32 -> f32, orders 1 and 3, fractional shifts, beside an rl_device_copy
                of as many bytes as the call has to move (the source read, the float64 intermediate written and read, the
                destination written; a copy of n bytes reads n and writes n)
  end to end    deconvolve_stack_registered against deconvolve_stack, 512 x 512 x 1 and x 4 views, K = 20, --frames uint16 frames,
                the same batch, page-locked input: wall times of the whole calls, set-up included, and the share of the registered
                call that is not in the unregistered one (registration and the transfers that are not overlapped)

each warmed once, then --repeats samples: the median and the spread (min, max) of a host clock around work that ends in a device
synchronise.

With --pipeline, instead (profiles/register_pipeline/throughput.json):
  estimate      the estimate alone on 256 pairs of 512 x 512 at R = 4 / 8 / 16, refine 1: the host's peak search against
                device_peaks (rl_register_estimate), alternating
  pipeline      the end-to-end workload above, 1 and 4 views, max_shift 8, refine 1, page-locked raw and out arrays: the host loop,
                the pipeline with f64 output, the pipeline with u16 output and deconvolve_stack, in one process in alternating order

    python tools/gpu/register_throughput.py [--repeats 5] [--frames 1024] [--pipeline] [--out profiles/register/throughput.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K, N, PAIRS = 20, 512, 256
DARK, GAIN = 100.0, 0.46


def samples(fn, sync, repeats):
    out = []
    for rep in range(repeats + 1):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep:
            out.append((time.perf_counter() - t0) * 1e3)
    return {'ms': float(np.median(out)), 'min_ms': float(min(out)), 'max_ms': float(max(out)), 'samples': len(out)}


def sums_rows(reg, repeats):
    dev = reg._Device(device=0)
    rng = np.random.default_rng(1)
    rows = {}
    try:
        imgs = dev.alloc((PAIRS + 1) * N * N, 'f32')
        dev.upload(imgs, (rng.random((PAIRS + 1, N, N)) * 100.0).astype(np.float32))
        ref_off, mov_off = [0] * PAIRS, [(k + 1) * N * N for k in range(PAIRS)]
        for R in (4, 8, 16):
            M = R
            row = samples(lambda: dev.sums(imgs, ref_off, imgs, mov_off, N, N, R, M), dev.ctx.synchronize, repeats)
            W, interior = 2 * R + 1, (N - 2 * M) ** 2
            fma = 2.0 * W * W * interior * PAIRS
            TY, nd = 16, W * W
            G = 1
            while nd < 256 and G * 2 <= TY and G * 2 * nd <= 256:
                G *= 2
            strips = -(-(N - 2 * M) // TY) * G
            part = PAIRS * strips * nd * 3 * 8
            moved = (PAIRS + 1) * N * N * 4 + 2 * part + PAIRS * nd * 3 * 8
            row.update({'pairs': PAIRS, 'R': R, 'M': M, 'fma': fma, 'fma_per_s': fma / row['ms'] * 1e3, 'bytes_moved': moved,
                        'gb_per_s': moved / row['ms'] / 1e6})
            rows['R=%d' % R] = row
    finally:
        dev.close()
    return rows


def shift_rows(reg, _lib, repeats):
    dev = reg._Device(device=0)
    rng = np.random.default_rng(2)
    n = PAIRS * N * N
    rows = {}
    try:
        src, dst = dev.alloc(n, 'f32'), dev.alloc(n, 'f32')
        spare_a, spare_b = dev.alloc(n * 3, 'f32'), dev.alloc(n * 3, 'f32')
        dev.upload(src, (rng.random((PAIRS, N, N)) * 100.0).astype(np.float32))
        shifts = rng.uniform(-3.0, 3.0, (PAIRS, 2))
        moved = n * (4 + 8 + 8 + 4)
        for order in (1, 3):
            row = samples(lambda: dev.shift(src, 0, PAIRS, N, N, shifts, order, 1e-9, dst), dev.ctx.synchronize, repeats)
            copy = samples(lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, spare_a.ptr, spare_b.ptr, moved // 2)), dev.ctx.synchronize, repeats)
            row.update({'images': PAIRS, 'order': order, 'bytes_moved': moved, 'gb_per_s': moved / row['ms'] / 1e6,
                        'copy_of_as_many_bytes_ms': copy['ms'], 'over_copy': row['ms'] / copy['ms']})
            rows['order=%d' % order] = row
    finally:
        dev.close()
    return rows


def frames_u16(F, V):
    """64 distinct Poisson frames of the 512 x 512 astronaut over a dark level of 100, view v and frame f displaced by whole pixels
    (np.roll: the drift costs nothing to build), repeated."""
    objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
    obj = np.kron(objs['astronaut'].astype(np.float64), np.ones((1, 4, 4)))[0]
    obj = 40.0 + obj * (900.0 / obj.max())
    rng = np.random.default_rng(7)
    base = np.empty((min(F, 64), V, N, N), dtype=np.uint16)
    for f in range(len(base)):
        for v in range(V):
            base[f, v] = DARK + rng.poisson(np.roll(obj, (f % 5 - 2 + v, 2 - f % 3 - v), axis=(0, 1)) / GAIN)
    return np.ascontiguousarray(np.tile(base, (-(-F // len(base)), 1, 1, 1))[:F])


def end_to_end(reg, stack, _lib, F, B, repeats):
    import bench
    psf = bench.workload(N)[1]
    rows = {}
    for V in (1, 4):
        psfs = [psf[0]] * V if V > 1 else psf
        raw = _lib.pinned_empty((F, V, N, N), np.uint16)
        raw[:] = frames_u16(F, V)
        cam = stack.CameraModel(dark=DARK, gain=GAIN, saturation=65535)
        none = lambda: None
        plain = samples(lambda: stack.deconvolve_stack(raw, psfs, K, camera=cam, dtype='f32', out_dtype='f32', batch=B), none, repeats)
        regd = samples(lambda: reg.deconvolve_stack_registered(raw, psfs, K, camera=cam, dtype='f32', batch=B), none, repeats)
        given = samples(lambda: reg.deconvolve_stack_registered(raw, psfs, K, camera=cam, dtype='f32', batch=B, shifts=np.zeros((F, V, 2))), none, repeats)
        rows['views=%d' % V] = {'deconvolve_stack': plain, 'registered': regd, 'registered_given_shifts': given, 'frames': F, 'batch': B,
                                'frames_per_s_plain': F / plain['ms'] * 1e3, 'frames_per_s_registered': F / regd['ms'] * 1e3,
                                'share_not_in_plain': 1.0 - plain['ms'] / regd['ms'],
                                'share_estimation': (regd['ms'] - given['ms']) / regd['ms']}
        del raw
    return rows


def alternating(legs, repeats):
    """Every leg warmed once, then `repeats` rounds in which each leg runs once, the order rotated from round to round (a drift of
    the machine over the run falls on every leg alike); wall times of calls that end in a synchronise."""
    names = list(legs)
    for name in names:
        legs[name]()
    out = {name: [] for name in names}
    for rep in range(repeats):
        for name in names[rep % len(names):] + names[:rep % len(names)]:
            t0 = time.perf_counter()
            legs[name]()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {'ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v)), 'samples': len(v)} for name, v in out.items()}


def pipeline_rows(reg, stack, _lib, F, B, repeats):
    """The README's workload (F uint16 frames of 512 x 512, K = 20, batch B, page-locked, max_shift 8, refine 1), 1 and 4 views:
    deconvolve_stack_registered's host loop, the pipeline with f64 output, the pipeline with u16 output, and deconvolve_stack, in
    one process in alternating order."""
    import bench
    psf = bench.workload(N)[1]
    rows = {}
    for V in (1, 4):
        psfs = [psf[0]] * V if V > 1 else psf
        raw = _lib.pinned_empty((F, V, N, N), np.uint16)
        raw[:] = frames_u16(F, V)
        out64, out16 = _lib.pinned_empty((F, N, N), np.float64), _lib.pinned_empty((F, N, N), np.uint16)
        cam = stack.CameraModel(dark=DARK, gain=GAIN, saturation=65535)
        kw = dict(camera=cam, dtype='f32', batch=B, max_shift=8, refine=1)
        legs = {'host_loop': lambda: reg.deconvolve_stack_registered(raw, psfs, K, **kw),
                'pipeline_f64': lambda: reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='f64', out=out64, **kw),
                'pipeline_u16': lambda: reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='u16', out=out16, **kw),
                'deconvolve_stack': lambda: stack.deconvolve_stack(raw, psfs, K, camera=cam, dtype='f32', out_dtype='u16', batch=B, out=out16)}
        row = alternating(legs, repeats)
        _, info = reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='u16', out=out16, **kw)
        row.update({'frames': F, 'batch': B, 'views': V, 'pipeline_times_ms': info['times_ms']})
        for name in legs:
            row[name]['frames_per_s'] = F / row[name]['ms'] * 1e3
        row['pipeline_u16_over_host_loop'] = row['host_loop']['ms'] / row['pipeline_u16']['ms']
        rows['views=%d' % V] = row
        print(json.dumps({'views=%d' % V: row}), flush=True)
        del raw, out64, out16
    return rows


def estimate_rows(reg, repeats):
    """The estimate alone, 256 pairs of 512 x 512 f32 against one reference, R = 4 / 8 / 16, margin R + 2, refine 1: the host's peak
    search (the sums come down) against device_peaks (5 doubles per pair come down), alternating."""
    dev = reg._Device(device=0)
    rng = np.random.default_rng(3)
    rows = {}
    try:
        imgs = dev.alloc((PAIRS + 1) * N * N, 'f32')
        dev.upload(imgs, (rng.random((PAIRS + 1, N, N)) * 100.0).astype(np.float32))
        scratch = dev.alloc(PAIRS * N * N, 'f64')
        ref_off, mov_off = [0] * PAIRS, [(k + 1) * N * N for k in range(PAIRS)]
        for R in (4, 8, 16):
            args = (dev, imgs, ref_off, imgs, mov_off, N, N, R, 1, R + 2, scratch)
            legs = {'host_peaks': lambda: reg._estimate(*args), 'device_peaks': lambda: reg._estimate_on_device(*args)}
            row = alternating(legs, repeats)
            row.update({'pairs': PAIRS, 'R': R, 'refine': 1, 'host_over_device': row['host_peaks']['ms'] / row['device_peaks']['ms']})
            rows['R=%d' % R] = row
    finally:
        dev.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--pipeline', action='store_true', help='only the pipeline and estimate legs (default output profiles/register_pipeline/)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib, registration as reg, stack
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    if args.pipeline:
        res = {'image': [N, N], 'iterations': K, 'repeats': args.repeats}
        res['estimate'] = estimate_rows(reg, args.repeats)
        print(json.dumps(res['estimate']), flush=True)
        res['pipeline'] = pipeline_rows(reg, stack, _lib, args.frames, args.batch, args.repeats)
        out = args.out or os.path.join(ROOT, 'profiles', 'register_pipeline', 'throughput.json')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        return
    args.out = args.out or os.path.join(ROOT, 'profiles', 'register', 'throughput.json')
    res = {'image': [N, N], 'iterations': K, 'repeats': args.repeats}
    res['sums'] = sums_rows(reg, args.repeats)
    print(json.dumps(res['sums']), flush=True)
    res['shift'] = shift_rows(reg, _lib, args.repeats)
    print(json.dumps(res['shift']), flush=True)
    res['end_to_end'] = end_to_end(reg, stack, _lib, args.frames, args.batch, max(1, args.repeats // 2))
    print(json.dumps(res['end_to_end']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
