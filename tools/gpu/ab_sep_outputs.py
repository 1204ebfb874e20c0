"""Manual helper (not a test): are the stencil plans of two library builds the same product?  Both libraries in ONE process (each
through its own copy of rescan_line_sted_amd._lib, as tools/gpu/ab_bench.py binds them); on a fixed list of plans -- the shapes of
tests/test_gpu_separable.py's separable / direct tests plus ten seeds of the shared random generator (tests/sep_reference.py), both
types, all forms -- forward, adjoint with and without the normaliser, the normaliser and five iterations must be BIT-IDENTICAL, and
strategy() and device_bytes equal.

    python3 tools/gpu/ab_sep_outputs.py LIB_A LIB_B          exit status 1 on any difference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), HERE]
from ab_bench import bind  # noqa: E402
import sep_reference as sr  # noqa: E402
import test_gpu_separable as tg  # noqa: E402


def fixed_list():
    """(label, form, psfs [V][py][px], frames, ny, nx)"""
    rng = np.random.default_rng(1)
    out = []
    for kind, shape in (('row7', (33, 70)), ('two_lines', (128, 128)), ('even_skew', (61, 300))):
        for form in ('one', 'two'):
            out.append(('%s %s' % (kind, form), form, np.stack(tg.rank1_views(kind)), 3) + shape)
    for py, px, V, shape in ((3, 5, 2, (40, 70)), (7, 7, 1, (128, 128)), (11, 9, 3, (61, 300)), (2, 6, 2, (33, 33)), (15, 13, 1, (200, 90)), (8, 4, 4, (17, 250))):
        out.append(('direct %dx%d' % (py, px), 'direct', rng.random((V, py, px)) + 0.05, 2) + shape)
    return out


def main():
    libs = sys.argv[1:3]
    mods = [bind(p, str(i)) for i, p in enumerate(libs)]
    emu = sr.Emulator()
    cases = []
    for label, form, psfs, B, ny, nx in fixed_list():
        rng = np.random.default_rng(len(cases))
        cases.append((label, form, psfs, B, ny, nx, rng.random((B, ny, nx)) * 50, rng.random((B, len(psfs), ny, nx)) + 0.5))
    for seed in range(10):
        for dtype in ('f32', 'f64'):
            c, psfs, _ = tg.plan_case(emu, seed, dtype)
            cases.append(('seed %d %s %s %dx%d taps' % (seed, c.form, dtype, c.py, c.px), c.form, psfs, c.frames, c.ny, c.nx, c.x.astype(np.float64),
                          c.aux.astype(np.float64)))
    bad = 0
    for label, form, psfs, B, ny, nx, x, y in cases:
        for dtype in ('f32', 'f64'):
            if label.startswith('seed') and dtype not in label:
                continue
            res = []
            for m in mods:
                plan = tg.forced_plan(m, form, psfs, B, ny, nx, dtype)
                plan.set_measurement(y)
                plan.iterate(5)
                res.append((plan.forward(x), plan.adjoint(y, True), plan.adjoint(y, False), plan.normalization(), plan.estimate(), plan.strategy(),
                            plan.info()['device_bytes']))
            same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res[0][:5], res[1][:5])) and res[0][5:] == res[1][5:]
            bad += not same
            print('%-34s %s  %s  device_bytes %d / %d  %s' % (label, dtype, 'bit-identical' if same else 'DIFFERENT', res[0][6], res[1][6],
                                                              {k: v for k, v in res[0][5].items() if v}), flush=True)
    print('%d plans compared, %d different' % (sum(1 for c in cases for d in ('f32', 'f64') if not (c[0].startswith('seed') and d not in c[0])), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
