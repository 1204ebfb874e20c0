#!/usr/bin/env python3
"""Throughput of the coarse registration stage (manual tool; INTEGRATION.md section 5i, DESIGN.md section 4k, README status table).

  xcorr         rl_register_xcorr at 512 x 512, 256 pairs (one reference, 256 moving images), f32, R in {16, 32, 64} (lengths 576 x
                576): the time of the whole call (five launches per chunk of pairs, the download of the fields; it ends in a
                synchronise) and the bytes the stage has to move -- both images read twice (statistics, row pass), the row spectra
                written and read, the kept rows written and read, the window written and read
  sums          rl_register_sums on the same pairs, R in {8, 16, 32}, M = R: the direct window the stage is compared with
  copy          an rl_device_copy of as many bytes as the stage has to move at R = 64 (a copy of n bytes reads n and writes n)
  end to end    deconvolve_stack_registered, 512 x 512 x 1 and x 4 views, K = 20, --frames uint16 frames, page-locked input, in three
                forms: coarse=None with max_shift=8; coarse=64 with max_shift=2; shifts= given (no estimation)

all in one process, each warmed once, then --repeats samples: the median and the spread (min, max) of a host clock around work that
ends in a device synchronise.  Writes the JSON and a short README.md beside it; reads nothing outside the repository.

    python tools/gpu/xcorr_throughput.py [--repeats 3] [--frames 1024] [--out profiles/xcorr/throughput.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from register_throughput import DARK, GAIN, K, N, PAIRS, frames_u16, samples  # noqa: E402

L = 576                                # the transform length of 512 + R for R <= 64


def stage_bytes(R):
    W = 2 * R + 1
    return PAIRS * (2 * (2 * N * N * 4) + 2 * N * L * 8 + 2 * W * L * 8 + 2 * W * W * 4)


def kernel_rows(reg, _lib, repeats):
    dev = reg._Device(device=0)
    rng = np.random.default_rng(1)
    rows = {'xcorr': {}, 'sums': {}}
    try:
        imgs = dev.alloc((PAIRS + 1) * N * N, 'f32')
        dev.upload(imgs, (rng.random((PAIRS + 1, N, N)) * 100.0).astype(np.float32))
        ref_off, mov_off = [0] * PAIRS, [(k + 1) * N * N for k in range(PAIRS)]
        for R in (16, 32, 64):
            row = samples(lambda: dev.xcorr(imgs, ref_off, imgs, mov_off, N, N, R), dev.ctx.synchronize, repeats)
            moved = stage_bytes(R)
            row.update({'pairs': PAIRS, 'R': R, 'lengths': [L, L], 'bytes_moved': moved, 'gb_per_s': moved / row['ms'] / 1e6})
            rows['xcorr']['R=%d' % R] = row
        for R in (8, 16, 32):
            row = samples(lambda: dev.sums(imgs, ref_off, imgs, mov_off, N, N, R, R), dev.ctx.synchronize, repeats)
            row.update({'pairs': PAIRS, 'R': R, 'M': R})
            rows['sums']['R=%d' % R] = row
        moved = stage_bytes(64)
        a, b = dev.alloc(moved // 8, 'f32'), dev.alloc(moved // 8, 'f32')
        copy = samples(lambda: _lib.check(_lib.lib.rl_device_copy(dev.ctx.handle, a.ptr, b.ptr, moved // 2)), dev.ctx.synchronize, repeats)
        copy.update({'bytes_moved': moved, 'gb_per_s': moved / copy['ms'] / 1e6})
        rows['copy_of_the_bytes_at_R=64'] = copy
        rows['xcorr_over_copy_at_R=64'] = rows['xcorr']['R=64']['ms'] / copy['ms']
    finally:
        dev.close()
    return rows


def end_to_end(reg, stack, _lib, F, B, repeats):
    import bench
    psf = bench.workload(N)[1]
    rows = {}
    none = lambda: None
    for V in (1, 4):
        psfs = [psf[0]] * V if V > 1 else psf
        raw = _lib.pinned_empty((F, V, N, N), np.uint16)
        raw[:] = frames_u16(F, V)
        cam = stack.CameraModel(dark=DARK, gain=GAIN, saturation=65535)
        run = lambda **kw: reg.deconvolve_stack_registered(raw, psfs, K, camera=cam, dtype='f32', batch=B, **kw)
        window = samples(lambda: run(max_shift=8), none, repeats)
        coarse = samples(lambda: run(coarse=64, max_shift=2), none, repeats)
        given = samples(lambda: run(shifts=np.zeros((F, V, 2))), none, repeats)
        s_w, s_c = run(max_shift=8)[1]['shifts'], run(coarse=64, max_shift=2)[1]['shifts']
        rows['views=%d' % V] = {'window_max_shift_8': window, 'coarse_64_max_shift_2': coarse, 'given_shifts': given, 'frames': F, 'batch': B,
                                'estimation_ms_window': window['ms'] - given['ms'], 'estimation_ms_coarse': coarse['ms'] - given['ms'],
                                'largest_difference_of_the_two_estimates_px': float(np.abs(s_w - s_c).max())}
        del raw
    return rows


README = """# Coarse registration stage: throughput

`throughput.json` is written by `tools/gpu/xcorr_throughput.py` on one MI355X: all runs in one process, each warmed once, a host
clock around calls that end in a device synchronise, the median of {repeats} samples (with minimum and maximum).

| 256 pairs of 512 x 512, f32 | ms |
|---|---|
{table}

End to end ({frames} uint16 frames, K = 20, batch {batch}; whole calls, set-up included):

| views | window, max_shift = 8 | coarse = 64, max_shift = 2 | shifts given |
|---|---|---|---|
{e2e}

DESIGN.md section 4k reads these figures.
"""


def write_readme(path, res):
    k = res['kernels']
    lines = ['| rl_register_xcorr R = %s | %.2f |' % (r.split('=')[1], v['ms']) for r, v in k['xcorr'].items()]
    lines += ['| rl_register_sums R = %s | %.2f |' % (r.split('=')[1], v['ms']) for r, v in k['sums'].items()]
    lines += ['| rl_device_copy of the bytes the stage moves at R = 64 (%.2f GB) | %.2f |' % (k['copy_of_the_bytes_at_R=64']['bytes_moved'] / 1e9,
                                                                                              k['copy_of_the_bytes_at_R=64']['ms'])]
    e2e = ['| %s | %.0f ms | %.0f ms | %.0f ms |' % (v.split('=')[1], r['window_max_shift_8']['ms'], r['coarse_64_max_shift_2']['ms'], r['given_shifts']['ms'])
           for v, r in res.get('end_to_end', {}).items()]
    frames = next(iter(res['end_to_end'].values()))['frames'] if res.get('end_to_end') else 0
    batch = next(iter(res['end_to_end'].values()))['batch'] if res.get('end_to_end') else 0
    with open(path, 'w') as f:
        f.write(README.format(repeats=res['repeats'], table='\n'.join(lines), e2e='\n'.join(e2e), frames=frames, batch=batch))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'xcorr', 'throughput.json'))
    args = ap.parse_args()
    from rescan_line_sted_amd import _lib, registration as reg, stack
    if _lib.device_count() < 1:
        sys.exit('no GPU: the throughput is not measured')
    res = {'image': [N, N], 'iterations': K, 'repeats': args.repeats}
    res['kernels'] = kernel_rows(reg, _lib, args.repeats)
    print(json.dumps(res['kernels']), flush=True)
    res['end_to_end'] = end_to_end(reg, stack, _lib, args.frames, args.batch, args.repeats)
    print(json.dumps(res['end_to_end']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    write_readme(os.path.join(os.path.dirname(os.path.abspath(args.out)), 'README.md'), res)


if __name__ == '__main__':
    main()
