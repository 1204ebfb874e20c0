#!/usr/bin/env python3
"""Total-variation regularised Richardson-Lucy against plain, on the device (manual study):

  * device ms per frame-iteration, plain and regularised (rl_deconv_last_ms of one rl_deconv_iterate over a batch), on
    512^2 x 1 view f32 (the pair loop), 512^2 x 4 views f32, 512^2 x 1 view f64 and 2048^2 x 4 views f32 (the split pass);
    with --parent LIB also the plain iteration of that build, bound in the same process
  * --ab LIB: iterate(20) with the regulariser off, bit for bit against that build on eight plan shapes
  * the fabric bytes of a frame-iteration from two counter passes

Object: the astronaut, each pixel repeated, 5e10 photons per 128^2, Philox noise; lambda = 0.01, eps_rel = 0.1.

    python tools/gpu/tv_study.py [--parent LIB] [--ab LIB] [--out FILE]
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python tools/gpu/tv_study.py --pmc-pass CONFIG --mode tv
    python tools/gpu/tv_study.py --traffic FETCH.csv WRITE.csv --pmc-pass CONFIG   # bytes per frame-iteration of such a pass
      (RL-loop kernels only; FETCH_SIZE doubled as in tools/pmc_traffic.py; 5 + 3 x 5 iterations of the config's batch)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from rescan_line_sted_amd import _lib  # noqa: E402
from ab_bench import bind  # noqa: E402

LAM, EPS = 0.01, 0.1
POINT, LINE = '1p5x_lr/point_sted_psf', '2p0x_lr/line_sted_psfs'
CONFIGS = {'512x1_f32': (POINT, 512, 64, 'f32'), '512x4_f32': (LINE, 512, 16, 'f32'), '512x1_f64': (POINT, 512, 16, 'f64'),
           '2048x4_f32': (LINE, 2048, 2, 'f32')}


def _gauss(n, s):
    x = np.arange(n) - (n - 1) / 2
    return np.exp(-x ** 2 / (2 * s * s))


def inputs(psf_name, n):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g8_fig2_psfs.npz'))
    o = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))['astronaut'][0].astype(np.float64)
    o = np.kron(o, np.ones((-(-n // 128), -(-n // 128))))[:n, :n]
    if psf_name == 'separable':
        return [np.outer(_gauss(7, 1.2), _gauss(5, 0.9))[None], np.outer(_gauss(5, 0.8), _gauss(7, 1.5))[None]], o
    return list(g[psf_name]), o


def ms_per_frame_iteration(mod, psfs, obj, n, dtype, tv, B, K=20, runs=3):
    plan = mod.DeconvPlan(psfs, B, n, n, dtype=dtype)
    if tv:
        plan.set_tv(LAM, EPS)
    plan.set_object(np.repeat(obj[None], B, axis=0), 5e10 * (n / 128) ** 2)
    plan.simulate(seed=1)
    plan.iterate(K)                       # warm-up
    best = float('inf')
    for _ in range(runs):
        plan.iterate(K)
        best = min(best, plan.last_ms()['iterate_ms'])
    return best / (B * K), plan.info()['device_bytes']


AB_SHAPES = [('512^2 V=1 f32 B=8 (pairs)', POINT, 512, 8, 'f32', None), ('512^2 V=4 f32 B=4', LINE, 512, 4, 'f32', None),
             ('512^2 V=1 f64 B=2', POINT, 512, 2, 'f64', None), ('2048^2 V=4 f32 B=2 (split)', LINE, 2048, 2, 'f32', None),
             ('128^2 V=1 f32 B=4', POINT, 128, 4, 'f32', None), ('128^2 V=4 f64 B=3', LINE, 128, 3, 'f64', None),
             ('512^2 separable f32 B=2', 'separable', 512, 2, 'f32', None), ('200^2 V=1 f32 B=4 accelerated', POINT, 200, 4, 'f32', 'biggs-andrews')]


def ab(parent, emit):
    old = bind(parent, 'parent')
    for name, psf_name, n, B, dtype, accel in AB_SHAPES:
        psfs, obj = inputs(psf_name, n)
        est, nbytes = [], []
        for mod in (old, _lib):
            plan = mod.DeconvPlan(psfs, B, n, n, dtype=dtype, acceleration=accel)
            nbytes.append(plan.info()['device_bytes'])
            plan.set_object(np.repeat(obj[None], B, axis=0), 5e10 * (n / 128) ** 2)
            plan.simulate(seed=5)
            plan.iterate(20)
            est.append(plan.estimate())
        emit('%-32s iterate(20) with the regulariser off bit-identical to the parent build: %s   device_bytes parent %d new %d'
             % (name, np.array_equal(est[0], est[1]), nbytes[0], nbytes[1]))


def traffic(fetch, write, config, emit):
    import csv
    import re
    tot = {}
    for path, counter, scale in ((fetch, 'FETCH_SIZE', 2.0), (write, 'WRITE_SIZE', 1.0)):
        with open(path) as f:
            for r in csv.DictReader(f):
                if r['Counter_Name'] == counter and re.search(r'k_rowpass|k_rowpair|k_colconv|k_tv|k_sep', r['Kernel_Name']):
                    key = re.sub(r'[<(].*', '', r['Kernel_Name'].split('::')[-1])
                    tot.setdefault(key, [0.0, 0.0])[0 if counter == 'FETCH_SIZE' else 1] += scale * float(r['Counter_Value']) * 1024
    fi = CONFIGS[config][2] * 20
    for k, (rd, wr) in sorted(tot.items()):
        emit('%-22s read %.3f MB write %.3f MB per frame-iteration' % (k, rd / fi / 1e6, wr / fi / 1e6))
    emit('total %.3f MB per frame-iteration' % (sum(rd + wr for rd, wr in tot.values()) / fi / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent', default=None, help='a build of the parent commit: its plain iteration is timed too')
    ap.add_argument('--ab', default=None, help='a build of the parent commit: bit identity with the regulariser off')
    ap.add_argument('--pmc-pass', default=None, help='run CONFIG in one mode (20 iterations in all) and stop')
    ap.add_argument('--mode', default='tv', choices=('plain', 'tv'))
    ap.add_argument('--traffic', nargs=2, default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
    if a.traffic:
        traffic(a.traffic[0], a.traffic[1], a.pmc_pass, emit)
    elif a.pmc_pass:
        psf_name, n, B, dtype = CONFIGS[a.pmc_pass]
        psfs, obj = inputs(psf_name, n)
        ms_per_frame_iteration(_lib, psfs, obj, n, dtype, a.mode == 'tv', B, K=5)
    else:
        old = bind(a.parent, 'parent_t') if a.parent else None
        emit('# RL-TV against plain RL (device ms from rl_deconv_last_ms, best of 3 x iterate(20)); lambda %g eps_rel %g' % (LAM, EPS))
        for name, (psf_name, n, B, dtype) in CONFIGS.items():
            psfs, obj = inputs(psf_name, n)
            plain, b0 = ms_per_frame_iteration(_lib, psfs, obj, n, dtype, False, B)
            tv, b1 = ms_per_frame_iteration(_lib, psfs, obj, n, dtype, True, B)
            s = '%-11s B %3d ms/frame-iteration plain %.5f regularised %.5f (x%.2f)  device_bytes %d -> %d' % (name, B, plain, tv, tv / plain, b0, b1)
            if old:
                p, _ = ms_per_frame_iteration(old, psfs, obj, n, dtype, False, B)
                s += '  parent build plain %.5f (regularised / parent x%.2f)' % (p, tv / p)
            emit(s)
        if a.ab:
            ab(a.ab, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
