#!/usr/bin/env python3
"""Throughput of the affine registration path (manual tool; INTEGRATION.md section 5l, DESIGN.md section 4n, README status table).

  warp          rl_warp_images on 256 images of 512 x 512, f32 -> f32, a rotation by 1 degree about the centre plus a fractional
                translation, orders 1 and 3, beside an rl_device_copy of as many bytes as the call has to move (order 1: the source
                read, the destination written; order 3: also the two float64 intermediates written and read; a copy of n bytes
                reads n and writes n).  The split of order 3: the two FIR passes alone, timed as rl_shift_images order 3 f32 -> f64
                on the same images (the same kernel, 64 taps instead of the prefilter's 61), and the rest, the evaluation.  Also with
                every tile read directly (rl_warp_path 1).
  sums          rl_affine_sums on 256 pairs of 512 x 512, M = 8, an f32 reference shared by all and f64 warped images (what
                estimate_transforms hands it), beside a copy that moves as many bytes as the call has to read
  estimate      estimate_transforms, model 'rigid', 16 pairs of 512 x 512 (4 levels, 5 passes each): the whole call, uploads included
  end to end    deconvolve_stack_registered(model='rigid') against model='translation', 512 x 512 x 2 views, view 1 rotated by 1.5
                degrees, K = 20, --frames uint16 frames: wall times of the whole calls, set-up included

each warmed once, then --repeats samples: the median and the spread (min, max) of a host clock around work that ends in a device
synchronise.

    python tools/gpu/affine_throughput.py [--repeats 5] [--frames 128] [--out profiles/affine/throughput.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K, N, IMAGES = 20, 512, 256
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


def rotation(degrees, t=(0.0, 0.0)):
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), -np.sin(a), t[0]], [np.sin(a), np.cos(a), t[1]]])


def warp_rows(reg, _lib, repeats):
    dev = reg._Device(device=0)
    rng = np.random.default_rng(2)
    n = IMAGES * N * N
    rows = {}
    try:
        src, dst, wide = dev.alloc(n, 'f32'), dev.alloc(n, 'f32'), dev.alloc(n, 'f64')
        spare_a, spare_b = dev.alloc(n * 5, 'f32'), dev.alloc(n * 5, 'f32')
        dev.upload(src, (rng.random((IMAGES, N, N)) * 100.0).astype(np.float32))
        T = np.stack([rotation(1.0, rng.uniform(-3.0, 3.0, 2)) for _ in range(IMAGES)])
        xf = reg.transform_matrix_offset(T, (N, N))
        copy = lambda b: samples(lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, spare_a.ptr, spare_b.ptr, b // 2)), dev.ctx.synchronize, repeats)
        for order, per_pixel in ((1, 4 + 4), (3, 4 + 8 + 8 + 8 + 8 + 4)):
            moved = n * per_pixel
            row = samples(lambda: dev.warp(src, 0, IMAGES, N, N, xf, order, 1e-9, dst, 0, N, N), dev.ctx.synchronize, repeats)
            c = copy(moved)
            row.update({'images': IMAGES, 'order': order, 'bytes_moved': moved, 'gb_per_s': moved / row['ms'] / 1e6,
                        'copy_of_as_many_bytes_ms': c['ms'], 'over_copy': row['ms'] / c['ms']})
            _lib.check(_lib.lib.rl_warp_path(dev.ctx.handle, 1))
            try:
                row['direct_path_ms'] = samples(lambda: dev.warp(src, 0, IMAGES, N, N, xf, order, 1e-9, dst, 0, N, N), dev.ctx.synchronize, repeats)['ms']
            finally:
                _lib.check(_lib.lib.rl_warp_path(dev.ctx.handle, 0))
            if order == 3:
                fir = samples(lambda: dev.shift(src, 0, IMAGES, N, N, T[:, :, 2], 3, None, wide), dev.ctx.synchronize, repeats)
                fir_moved = n * (4 + 8 + 8 + 8)
                row.update({'fir_passes_ms': fir['ms'], 'fir_passes_over_copy': fir['ms'] / copy(fir_moved)['ms'],
                            'evaluation_ms': row['ms'] - fir['ms'], 'evaluation_over_copy': (row['ms'] - fir['ms']) / copy(n * (8 + 4))['ms']})
            rows['order=%d' % order] = row
    finally:
        dev.close()
    return rows


def sums_rows(reg, _lib, repeats):
    dev = reg._Device(device=0)
    rng = np.random.default_rng(1)
    try:
        ref, w = dev.alloc(N * N, 'f32'), dev.alloc(IMAGES * N * N, 'f64')
        spare_a, spare_b = dev.alloc(IMAGES * N * N, 'f64'), dev.alloc(IMAGES * N * N, 'f64')
        dev.upload(ref, (rng.random((N, N)) * 100.0).astype(np.float32))
        dev.upload(w, rng.random((IMAGES, N, N)) * 100.0)
        M = 8
        row = samples(lambda: dev.affine_sums(ref, [0] * IMAGES, w, [k * N * N for k in range(IMAGES)], N, N, M), dev.ctx.synchronize, repeats)
        read = IMAGES * N * N * (8 + 4)             # (the shared reference is read once per pair, mostly from cache)
        c = samples(lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, spare_a.ptr, spare_b.ptr, read // 2)), dev.ctx.synchronize, repeats)
        interior = (N - 2 * M) ** 2
        row.update({'pairs': IMAGES, 'M': M, 'bytes_read': read, 'gb_per_s': read / row['ms'] / 1e6, 'fma': 45.0 * interior * IMAGES,
                    'fma_per_s': 45.0 * interior * IMAGES / row['ms'] * 1e3, 'copy_moving_as_many_bytes_ms': c['ms'], 'over_copy': row['ms'] / c['ms']})
        return row
    finally:
        dev.close()


def scene(F, angle):
    """uint16 frames (F, 2, N, N): Poisson noise on the 512 x 512 astronaut over a dark level of 100, view 1 rotated by `angle`."""
    from scipy import ndimage
    objs = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))
    obj = np.kron(objs['astronaut'].astype(np.float64), np.ones((1, 4, 4)))[0]
    obj = ndimage.gaussian_filter(40.0 + obj * (900.0 / obj.max()), 1.5)
    c = (N - 1) / 2.0
    L = rotation(angle)[:, :2]
    views = [obj, ndimage.affine_transform(obj, np.linalg.inv(L), offset=np.array([c, c]) - np.linalg.inv(L) @ np.array([c, c]), order=3, mode='mirror')]
    rng = np.random.default_rng(7)
    base = np.stack([[DARK + rng.poisson(v / GAIN) for v in views] for _ in range(min(F, 16))]).astype(np.uint16)
    return np.ascontiguousarray(np.tile(base, (-(-F // len(base)), 1, 1, 1))[:F])


def estimate_row(reg, repeats):
    raw = scene(16, 1.5).astype(np.float32)
    row = samples(lambda: reg.estimate_transforms(raw[:, 1], raw[:, 0], model='rigid'), lambda: None, repeats)
    T, info = reg.estimate_transforms(raw[:, 1], raw[:, 0], model='rigid')
    row.update({'pairs': 16, 'model': 'rigid', 'levels': int(info['levels']), 'passes': 5,
                'angle_degrees_median': float(np.median(np.rad2deg(np.arctan2(T[:, 1, 0], T[:, 0, 0])))), 'last_step_px_max': float(info['step'].max())})
    return row


def end_to_end(reg, stack, _lib, F, B, repeats):
    import bench
    psf = bench.workload(N)[1]
    psfs = [psf[0]] * 2
    raw = _lib.pinned_empty((F, 2, N, N), np.uint16)
    raw[:] = scene(F, 1.5)
    cam = stack.CameraModel(dark=DARK, gain=GAIN, saturation=65535)
    none = lambda: None
    kw = dict(camera=cam, dtype='f32', batch=B)
    shift = samples(lambda: reg.deconvolve_stack_registered(raw, psfs, K, **kw), none, repeats)
    rigid = samples(lambda: reg.deconvolve_stack_registered(raw, psfs, K, model='rigid', **kw), none, repeats)
    _, info = reg.deconvolve_stack_registered(raw, psfs, K, model='rigid', **kw)
    given = samples(lambda: reg.deconvolve_stack_registered(raw, psfs, K, view_transforms=info['view_transforms'], **kw), none, repeats)
    L = info['view_transforms'][1]
    return {'translation': shift, 'rigid': rigid, 'rigid_given_view_transforms': given, 'frames': F, 'batch': B, 'views': 2,
            'rigid_over_translation': rigid['ms'] / shift['ms'], 'estimated_angle_degrees': float(np.rad2deg(np.arctan2(L[1, 0], L[0, 0])))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'affine', 'throughput.json'))
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib, registration as reg, stack
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    res = {'image': [N, N], 'iterations': K, 'repeats': args.repeats}
    for name, fn in (('warp', lambda: warp_rows(reg, _lib, args.repeats)), ('sums', lambda: sums_rows(reg, _lib, args.repeats)),
                     ('estimate', lambda: estimate_row(reg, max(1, args.repeats // 2))),
                     ('end_to_end', lambda: end_to_end(reg, stack, _lib, args.frames, args.batch, max(1, args.repeats // 2)))):
        res[name] = fn()
        print(json.dumps({name: res[name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
