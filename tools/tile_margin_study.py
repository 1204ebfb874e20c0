"""How large must the margin of tiled Richardson-Lucy be?  (runs on the CPU, oracle only.)

For every figure-2 PSF set of tests/golden/g8_fig2_psfs.npz and g8b_fig2_psfs_more.npz: the cat object repeated 2 x 2 (320 x 320),
about 100 photons per pixel, tile 192, margins 0, 8, ..., 64 with the default overlap 2 * margin + 16 (the layout rule then gives
2 x 2 tiles up to margin 24, 3 x 3 up to 56, 4 x 4 at 64), K = 20 and K = 100 plain Richardson-Lucy iterations.  Recorded:

  * the normwise and the pixelwise (pixels above 1e-3 of the maximum) deviation of the tiled oracle from the whole-image oracle;
  * the normwise difference between the whole-image estimates of two noise seeds: the shot-noise floor of an estimate.

The overlap 2 * margin + 16 moves the tile edges with the margin, so a control series keeps the overlap at 144 -- 4 x 4 tiles at
origins 0, 42, 85, 128 for every margin: there the margin alone varies ('margins_fixed_origins').

The default margin is the smallest multiple of 8 whose K = 20 normwise deviation stays below 1 % of that floor for every set.  If
no margin of the study reaches every set (a PSF as wide as the un-depleted one carries the tile border far into the tile), it is
the smallest margin that reaches as many sets as any margin does, and the sets it does not reach are listed.

    python tools/tile_margin_study.py [--jobs N] [--out profiles/tiled/margin_study.json]
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import tile_reference as tr                        # noqa: E402
from oracle import line_sted_oracle as orc         # noqa: E402

TILE = 192
MARGINS = tuple(range(0, 65, 8))
KS = (20, 100)
FIXED_OVERLAP = 2 * max(MARGINS) + 16     # the control series: 4 x 4 tiles at the same origins for every margin
PHOTONS_PER_PIXEL = 100.0


def psf_sets():
    out = []
    for name in ('g8_fig2_psfs', 'g8b_fig2_psfs_more'):
        g = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
        for key in g.files:
            if key.endswith('_psf') or key.endswith('_psfs'):
                out.append((key, [np.asarray(p, dtype=np.float64) for p in g[key]]))
    return out


def snapshots(measurement, psfs):
    """{K: estimate} of one (V, ny, nx) measurement after each count of KS, in one run from ones."""
    d = orc.Deconvolver(psfs)
    d.noisy_measurement = [np.array(m, dtype=np.float64)[None] for m in measurement]
    out = {}
    for k in range(1, max(KS) + 1):
        d.iterate()
        if k in KS:
            out[k] = d.estimate[0].copy()
    return out


def study(item):
    key, psfs = item
    cat = np.load(os.path.join(ROOT, 'tests', 'golden', 'objects.npz'))['cat'].astype(np.float64)
    obj = np.tile(cat, (1, 2, 2))
    d = orc.Deconvolver(psfs)
    d.create_data_from_object(obj, total_brightness=PHOTONS_PER_PIXEL * obj.size, random_seed=0)
    noiseless = np.stack([m[0] for m in d.noiseless_measurement])
    seeds = []
    for seed in (0, 1):
        rng = np.random.RandomState(seed)
        seeds.append(rng.poisson(noiseless) + 1e-9)
    whole = [snapshots(m, psfs) for m in seeds]
    floor = {k: tr.normwise(whole[1][k], whole[0][k]) for k in KS}
    cache = {}                                      # a tile's estimates depend on its window alone

    def series(overlap_of):
        rows = []
        for margin in MARGINS:
            overlap = overlap_of(margin)
            lay = tr.Layout(obj.shape[-2:], TILE, overlap, margin)
            row = {'margin': margin, 'overlap': overlap, 'tiles': [len(lay.origins_y), len(lay.origins_x)]}
            tiles = {k: np.empty((1, len(lay.origins_y), len(lay.origins_x)) + lay.tile_shape) for k in KS}
            for iy, ay in enumerate(lay.origins_y):
                for ix, ax in enumerate(lay.origins_x):
                    w = (int(ay), int(ax))
                    if w not in cache:
                        cache[w] = snapshots(seeds[0][:, ay:ay + TILE, ax:ax + TILE], psfs)
                    for k in KS:
                        tiles[k][0, iy, ix] = cache[w][k]
            for k in KS:
                est = tr.blend(tiles[k], lay)[0]
                row['k%d' % k] = {'normwise': tr.normwise(est, whole[0][k]), 'pixelwise': tr.pixelwise(est, whole[0][k])}
            rows.append(row)
        return rows
    rows = series(lambda m: 2 * m + 16)
    fixed = series(lambda m: FIXED_OVERLAP)
    return {'psf_set': key, 'views': len(psfs), 'psf_shape': list(psfs[0].shape[-2:]),
            'shot_noise_floor_normwise': {'k%d' % k: floor[k] for k in KS}, 'margins': rows, 'margins_fixed_origins': fixed}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tiled', 'margin_study.json'))
    ap.add_argument('--sets', default=None, help='comma-separated substrings of the PSF set names to keep')
    args = ap.parse_args()
    items = psf_sets()
    if args.sets:
        items = [it for it in items if any(s in it[0] for s in args.sets.split(','))]
    items.sort(key=lambda it: -len(it[1]))
    with multiprocessing.Pool(args.jobs) as pool:
        results = pool.map(study, items, chunksize=1)
    results.sort(key=lambda r: r['psf_set'])
    def choose(series):
        passes = {m: sorted(r['psf_set'] for r in results for row in r[series]
                            if row['margin'] == m and row['k20']['normwise'] < 0.01 * r['shot_noise_floor_normwise']['k20']) for m in MARGINS}
        most = max(len(v) for v in passes.values())
        return min(m for m in MARGINS if len(passes[m]) == most), passes      # every set where one margin reaches every set
    default, passes = choose('margins')
    control, control_passes = choose('margins_fixed_origins')
    failing = sorted(set(r['psf_set'] for r in results) - set(passes[default]))
    doc = {'object': 'cat repeated 2 x 2 (320 x 320)', 'photons_per_pixel': PHOTONS_PER_PIXEL, 'tile': TILE, 'iterations': list(KS),
           'rule': 'smallest margin whose K = 20 normwise deviation is below 1 % of the shot-noise floor for every set; where no '
                   'margin of the study reaches every set: the smallest one that reaches as many sets as any margin does',
           'default_margin': default, 'default_overlap': 2 * default + 16, 'sets_not_reached_by_the_default': failing,
           'sets_within_1_percent_of_the_floor': {str(m): passes[m] for m in MARGINS},
           'fixed_origins': {'overlap': FIXED_OVERLAP, 'margin_by_the_same_rule': control,
                             'sets_within_1_percent_of_the_floor': {str(m): control_passes[m] for m in MARGINS}}, 'sets': results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('margin | worst K = 20 normwise deviation | worst deviation / floor')
    for margin in MARGINS:
        cells = [(row['k20']['normwise'], row['k20']['normwise'] / r['shot_noise_floor_normwise']['k20'])
                 for r in results for row in r['margins'] if row['margin'] == margin]
        print('%6d | %.3e | %.4f' % (margin, max(c[0] for c in cells), max(c[1] for c in cells)))
    print('fixed origins (overlap %d): margin | worst K = 20 deviation / floor over the sets the default reaches' % FIXED_OVERLAP)
    for margin in MARGINS:
        print('%6d | %.4f' % (margin, max(row['k20']['normwise'] / r['shot_noise_floor_normwise']['k20'] for r in results
                                          if r['psf_set'] not in failing for row in r['margins_fixed_origins'] if row['margin'] == margin)))
    print('the same rule at fixed origins:', control)
    print('default margin:', default, '-- sets it does not reach:', failing or 'none')


if __name__ == '__main__':
    main()
