#!/usr/bin/env python3
"""Biggs-Andrews accelerated Richardson-Lucy against plain, on the device (manual study):

  * device ms per frame-iteration, plain and accelerated (rl_deconv_last_ms of one rl_deconv_iterate over a batch)
  * the iterations and device time each mode needs to reach plain Richardson-Lucy's K = 128 I-divergence
    sum m log(m / Hx) - m + Hx (summed over views; formed on the device: DeconvPlan.divergence)

for 512^2 x 1 view (the 1.5x point PSF) and 512^2 x 4 views (the 2.0x line set), f32 and f64.  Object: the astronaut,
each pixel repeated 4 x 4, 5e10 photons per 128^2, Philox noise.

    python tools/gpu/accel_study.py [--batch 16] [--out profiles/r05/accel.log]
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python tools/gpu/accel_study.py --pmc-pass CONFIG --mode accel
    python tools/gpu/accel_study.py --traffic FETCH.csv WRITE.csv      # fabric bytes per frame-iteration of such a pass
      (RL-loop kernels only; FETCH_SIZE doubled as in tools/pmc_traffic.py; 20 iterations of 16 frames, the one H(obj) of the
      simulation included: ~1/20 of an iteration)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from rescan_line_sted_amd._lib import DeconvPlan  # noqa: E402

BA = 'biggs-andrews'
CONFIGS = {'1view_f32': ('1p5x_lr/point_sted_psf', 'f32'), '1view_f64': ('1p5x_lr/point_sted_psf', 'f64'),
           '4views_f32': ('2p0x_lr/line_sted_psfs', 'f32'), '4views_f64': ('2p0x_lr/line_sted_psfs', 'f64')}
N = 512


def inputs(psf_name):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g8_fig2_psfs.npz'))
    o = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))['astronaut'][0].astype(np.float64)
    return list(g[psf_name]), np.kron(o, np.ones((N // 128, N // 128)))


def ms_per_frame_iteration(psfs, obj, dtype, accel, B, K=20):
    plan = DeconvPlan(psfs, B, N, N, dtype=dtype, acceleration=accel)
    plan.set_object(np.repeat(obj[None], B, axis=0), 5e10 * (N / 128) ** 2)
    plan.simulate(seed=1)
    plan.iterate(K)                       # warm-up (and the history is under way)
    best = float('inf')
    for _ in range(3):
        plan.iterate(K)
        best = min(best, plan.last_ms()['iterate_ms'])
    return best / (B * K)


def to_quality(psfs, obj, dtype):
    """(target, plain iterations, accelerated iterations to reach it or None)"""
    out = {}
    for accel in (None, BA):
        plan = DeconvPlan(psfs, 1, N, N, dtype=dtype, acceleration=accel)
        plan.set_object(obj[None], 5e10 * (N / 128) ** 2)
        plan.simulate(seed=1)
        if accel is None:
            plan.iterate(128)
            out['target'] = float(plan.divergence()[0])
            continue
        out['accel_k'] = None
        for k in range(1, 129):
            plan.iterate(1)
            if plan.divergence()[0] <= out['target']:
                out['accel_k'] = k
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--out', default=None)
    ap.add_argument('--pmc-pass', default=None, help='run CONFIG in one mode (20 iterations) and stop')
    ap.add_argument('--mode', default='accel', choices=('plain', 'accel'))
    ap.add_argument('--traffic', nargs=2, default=None)
    a = ap.parse_args()
    if a.pmc_pass:
        psf_name, dtype = CONFIGS[a.pmc_pass]
        psfs, obj = inputs(psf_name)
        ms_per_frame_iteration(psfs, obj, dtype, BA if a.mode == 'accel' else None, a.batch, K=5)
        return
    if a.traffic:
        import csv
        import re
        tot = {}
        for path, counter, scale in ((a.traffic[0], 'FETCH_SIZE', 2.0), (a.traffic[1], 'WRITE_SIZE', 1.0)):
            with open(path) as f:
                for r in csv.DictReader(f):
                    if r['Counter_Name'] == counter and re.search(r'k_rowpass|k_rowpair|k_colconv|k_accel|k_sep', r['Kernel_Name']):
                        key = re.sub(r'[<(].*', '', r['Kernel_Name'].split('::')[-1])
                        tot.setdefault(key, [0.0, 0.0])[0 if counter == 'FETCH_SIZE' else 1] += scale * float(r['Counter_Value']) * 1024
        fi = a.batch * 20
        for k, (rd, wr) in sorted(tot.items()):
            print('%-22s read %.2f MB write %.2f MB per frame-iteration' % (k, rd / fi / 1e6, wr / fi / 1e6))
        print('total %.2f MB per frame-iteration' % (sum(rd + wr for rd, wr in tot.values()) / fi / 1e6))
        return
    lines = ['# Biggs-Andrews accelerated RL against plain RL, %d^2, batch %d (device ms from rl_deconv_last_ms)' % (N, a.batch)]
    for name, (psf_name, dtype) in CONFIGS.items():
        psfs, obj = inputs(psf_name)
        plain = ms_per_frame_iteration(psfs, obj, dtype, None, a.batch)
        acc = ms_per_frame_iteration(psfs, obj, dtype, BA, a.batch)
        q = to_quality(psfs, obj, dtype)
        k = q['accel_k']
        t_plain, t_acc = 128 * plain, (k * acc if k else float('nan'))
        lines.append('%-10s ms/frame-iteration plain %.5f accelerated %.5f (x%.2f) | plain K=128 I-divergence %.4e: '
                     'accelerated reaches it at K=%s; time to it plain %.3f ms, accelerated %.3f ms per frame (%.2fx sooner)'
                     % (name, plain, acc, acc / plain, q['target'], k, t_plain, t_acc, t_plain / t_acc if k else float('nan')))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
