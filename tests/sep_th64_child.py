"""Child process of tests/test_gpu_separable.py::test_tile_height_64_per_pixel_in_a_fresh_process (RLSTED_SEP_TH is read once per
process; the parent sets it to 64 in this process's environment).  f32 plans of the one-kernel and DIRECT forms on cases of the shared
generator; one JSON line per case: the worst error / bound of forward and adjoint against the long-double reference."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
import sep_reference as sr  # noqa: E402
from test_gpu_separable import forced_plan, plan_case  # noqa: E402
from rescan_line_sted_amd import _lib  # noqa: E402


def worst(out, ref, bound):
    err = np.abs(np.asarray(out, dtype=sr.LD) - ref)
    if np.any(err[bound == 0] != 0):
        return float('inf')
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def main():
    emu = sr.Emulator()
    done = 0
    for seed in range(40):
        if seed % 3 == 0:          # the two-pass form has one tile height
            continue
        c, psfs, views = plan_case(emu, seed, 'f32')
        if not emu.fits(c.form, 4, 64, c.V, views.py, views.px):
            continue
        plan = forced_plan(_lib, c.form, psfs, c.frames, c.ny, c.nx, 'f32')
        s = plan.strategy()
        conv, e, _ = sr.forward_ref(c.x, views, c.dtype)
        h = plan.forward(c.x)
        cv, ev, _ = sr.forward_views_ref(c.y, views, c.dtype)
        S = np.maximum(cv, 0).sum(axis=1)
        E = sr.sum_bound(S, ev.sum(axis=1), c.V, c.dtype)
        ht = plan.adjoint(c.y, False)
        print(json.dumps({'seed': seed, 'form': c.form, 'ny': c.ny, 'nx': c.nx, 'py': views.py, 'px': views.px, 'V': c.V, 'frames': c.frames,
                          'signed': c.signed, 'tile_height_env': os.environ.get('RLSTED_SEP_TH'), 'stencil': bool(s['separable'] or s['direct_stencil']),
                          'nan': bool(np.isnan(h).any() or np.isnan(ht).any()),
                          'forward': worst(h, np.maximum(conv, 0), e), 'adjoint': worst(ht, S, E)}), flush=True)
        done += 1
        if done == 10:
            break


if __name__ == '__main__':
    main()
