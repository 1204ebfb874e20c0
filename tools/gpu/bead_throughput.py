#!/usr/bin/env python3
"""Throughput of the bead measurement (manual tool; INTEGRATION.md section 5j, DESIGN.md section 4l, README status table).

  find_peaks    rl_find_peaks on 64 float32 images of 2048 x 2048 holding about 200 beads each, sigma 1 (h = 4), r = 3, border h + r,
                rel 0.2, cap 4096: the whole call (offsets and taps up, four launches, the candidates down, a synchronise), beside an
                rl_device_copy of the bytes the finder reads (the images once; a copy of n bytes reads n and writes n)
  measure_psfs  measure_psfs end to end on 8 frames x 4 views of 2048 x 2048 uint16, about 200 beads per image, size 21: the wall
                time of the call, split into ingest, detect (rl_find_peaks and the host's rejection), gather, align (the estimates
                and the shifts) and average (the means, the variance and what comes down) by a device synchronise after every step

each warmed once, then --repeats samples: the median and the spread (min, max) of a host clock around work that ends in a device
synchronise.  Writes the JSON and a README beside it.

    python tools/gpu/bead_throughput.py [--repeats 3] [--out profiles/beads/throughput.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, SIGMAS = 2048, ((1.3, 2.0), (2.0, 1.3), (1.6, 1.6), (1.2, 2.4))


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


def bead_image(rng, sy, sx, count=200, flux=5000.0, background=20.0, half=12):
    """Expected counts of one N x N image: `count` beads of the given widths at random sub-pixel centres on a jittered grid."""
    img = np.full((N, N), background)
    side = int(np.ceil(np.sqrt(count)))
    step = (N - 4 * half) / side
    k = np.arange(-half, half + 1)
    for i in range(count):
        cy = 2 * half + (i // side + 0.5) * step + rng.uniform(-0.3, 0.3) * step
        cx = 2 * half + (i % side + 0.5) * step + rng.uniform(-0.3, 0.3) * step
        iy, ix = int(cy), int(cx)
        gy = np.exp(-0.5 * ((iy + k - cy) / sy) ** 2)
        gx = np.exp(-0.5 * ((ix + k - cx) / sx) ** 2)
        img[iy - half:iy + half + 1, ix - half:ix + half + 1] += flux / (2.0 * np.pi * sy * sx) * np.outer(gy, gx)
    return img


def find_peaks_row(repeats):
    from rescan_line_sted_amd import beads
    from rescan_line_sted_amd._lib import check, lib
    import ctypes
    rng = np.random.default_rng(1)
    distinct = [rng.poisson(bead_image(rng, *SIGMAS[k % 4])).astype(np.float32) for k in range(8)]
    n, nbytes = 64, 64 * N * N * 4
    dev = beads._BeadDevice(device=0)
    try:
        imgs = dev.alloc(n * N * N, 'f32')
        for k in range(n):
            dev.upload(imgs, distinct[k % 8], k * N * N * 4)
        dst = dev.alloc(n * N * N, 'f32')
        w, h = beads.gaussian_taps(1.0)
        offs = [k * N * N for k in range(n)]
        found = {}

        def run():
            found['r'] = dev.find_peaks(imgs, offs, N, N, w, 3, h + 3, 0.2, 0.0, 4096)
        sync = dev.ctx.synchronize
        t = samples(run, sync, repeats)
        c = samples(lambda: check(lib.rl_device_copy(dev.ctx.handle, dst.ptr, imgs.ptr, ctypes.c_size_t(nbytes))), sync, repeats)
        counts = found['r'][1]
        return {'images': n, 'shape': [N, N], 'dtype': 'f32', 'sigma': 1.0, 'h': h, 'r': 3, 'border': h + 3, 'rel': 0.2, 'cap': 4096,
                'bytes_read': nbytes, 'find_peaks': t, 'copy_same_bytes': c, 'ratio_to_copy': t['ms'] / c['ms'],
                'candidates_per_image': [int(counts.min()), int(counts.max())]}
    finally:
        dev.close()


STAGES = {'ingest': 'ingest', 'find_peaks': 'detect', 'gather': 'gather', 'estimate': 'align', 'shift': 'align', 'group_stats': 'average',
          'download': 'average'}


def measure_row(repeats):
    from rescan_line_sted_amd import beads
    from rescan_line_sted_amd.stack import CameraModel
    rng = np.random.default_rng(2)
    F, V = 8, 4
    raw = np.empty((F, V, N, N), dtype=np.uint16)
    for f in range(F):
        for v in range(V):
            raw[f, v] = np.minimum(rng.poisson(bead_image(rng, *SIGMAS[v])) + 100, 65535)
    split = {}

    class Timed(beads._BeadDevice):
        pass
    for name, stage in STAGES.items():
        def wrap(fn, stage=stage):
            def call(self, *a, **k):
                t0 = time.perf_counter()
                r = fn(self, *a, **k)
                self.ctx.synchronize()
                split[stage] = split.get(stage, 0.0) + (time.perf_counter() - t0) * 1e3
                return r
            return call
        setattr(Timed, name, wrap(getattr(beads._BeadDevice, name)))
    keep = beads._Device
    beads._Device = Timed
    cam = CameraModel(dark=100.0, gain=1.0)
    runs, info = [], {}
    try:
        for rep in range(repeats + 1):
            split.clear()
            t0 = time.perf_counter()
            _, info = beads.measure_psfs(raw, 21, camera=cam)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                runs.append(dict(split, wall=wall))
    finally:
        beads._Device = keep
    med = {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in ('wall', 'ingest', 'detect', 'gather', 'align', 'average')}
    med['other'] = med['wall'] - sum(med[k] for k in ('ingest', 'detect', 'gather', 'align', 'average'))
    return {'frames': F, 'views': V, 'shape': [N, N], 'raw': 'uint16', 'size': 21, 'beads_per_image': 200, 'n_beads': info['n_beads'].tolist(),
            'rejected': info['rejected'], 'median_ms': med, 'samples': runs, 'upload_bytes': int(raw.nbytes)}


def readme(res):
    a, b = res['find_peaks'], res['measure_psfs']
    m = b['median_ms']
    h, r, taps = a['h'], a['r'], 2 * a['h'] + 1
    loads = ((16 + 2 * h) * 32 * taps / 512.0, (16 + 2 * r + 2 * h) * (32 + 2 * r) * taps / 512.0)      # per pixel of a 16 x 32 tile
    return '\n'.join([
        '# The bead measurement',
        '',
        '`python tools/gpu/bead_throughput.py --repeats %d` on one MI355X (`throughput.json`). Host clock around whole calls that end in a '
        'synchronise; each leg warmed once; medians, with the spread in `throughput.json`.' % res['repeats'],
        '',
        '**rl_find_peaks.** 64 f32 images of 2048², about 200 beads each, sigma 1 (h = 4), r = 3: %.2f ms (%.2f – %.2f) for the whole call. '
        'An `rl_device_copy` of the %.2f GiB it reads takes %.2f ms, so the finder runs at **%.2f×** a copy.'
        % (a['find_peaks']['ms'], a['find_peaks']['min_ms'], a['find_peaks']['max_ms'], a['bytes_read'] / 2 ** 30, a['copy_same_bytes']['ms'],
           a['ratio_to_copy']),
        '',
        'The project\'s streaming kernels sit at 1.1 – 4.2× a copy; where this one spends the rest, from the code (`csrc/bead_kernels.hpp`, '
        '`bp_row_body`, `bp_u`): the row pass reads the image from global memory tap by tap, not from a staged tile, and it runs twice, once '
        'for the levels (`k_peaks_range`) and once with the halo of h + r for the rule (`k_peaks_mark`). Per pixel of a 16 × 32 tile that is '
        '%.1f + %.1f = %.1f load instructions of one element against the single load of a copy (they hit the caches: the HBM traffic is the '
        'images twice plus halos). The tap count is a run-time value, so the compiled loop is not unrolled: one load, one wait for it '
        '(`s_waitcnt vmcnt(0)`), one `v_mul_f64` and one `v_add_f64` per tap, the tap itself through a scalar load — every one of a thread\'s '
        '%d-tap chains pays the full load latency %d times, and only the 8 workgroups a CU holds hide it. The float64 work (two operations '
        'per tap and pass, no contraction by definition) is some 30 GFLOP per call and far from a limit. `k_peaks_levels` and '
        '`k_peaks_compact` use one workgroup of 256 threads per image (64 of 256 CUs here; compact walks %d mask words per thread, '
        'uncoalesced, and thread 0 forms the 256-entry prefix alone); `kernel_split.md` has the measured split between the four kernels. '
        'Known, not done: staging the raw tile in LDS once (one coalesced load per pixel and halo pixel), keeping s of the RANGE pass for '
        'MARK instead of forming it again, and more than one workgroup per image in LEVELS / COMPACT.'
        % (loads[0], loads[1], loads[0] + loads[1], taps, taps, -(-(a['shape'][0] - 2 * a['border']) * -(-(a['shape'][1] - 2 * a['border']) // 32) // 256)),
        '',
        '**measure_psfs.** 8 frames × 4 views of 2048² uint16, about 200 beads per image, size 21: %.0f ms per call. ingest %.0f ms, '
        'detect %.0f ms, gather %.1f ms, align %.0f ms, average %.0f ms, the rest (the upload of %.0f MiB of raw data and host work) %.0f ms. '
        'Beads accepted per view: %s.'
        % (m['wall'], m['ingest'], m['detect'], m['gather'], m['align'], m['average'], b['upload_bytes'] / 2 ** 20, m['other'],
           ', '.join(str(k) for k in b['n_beads'])),
        ''])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'beads', 'throughput.json'))
    a = ap.parse_args()
    res = {'repeats': a.repeats, 'find_peaks': find_peaks_row(a.repeats), 'measure_psfs': measure_row(a.repeats)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(os.path.dirname(a.out), 'README.md'), 'w') as f:
        f.write(readme(res))
    print(json.dumps({k: (v['ratio_to_copy'] if k == 'find_peaks' else v['median_ms']) for k, v in res.items() if k != 'repeats'}))


if __name__ == '__main__':
    main()
