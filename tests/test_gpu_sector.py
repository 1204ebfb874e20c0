"""The angle-resolved ring statistics on the MI355X (include/rlsted.h rl_ring_sector_stats): parity with numpy and the exact sector
oracle (tests/sector_reference.py) under the derived bound, batch independence bit for bit, gratings that pin the axis order and the
sign of the angle, the sector sums against rl_ring_stats, the Python layer on a sweep's device-resident estimates, and the error
codes."""
import ctypes
import os

import numpy as np
import pytest

import ring_reference as rr
import sector_reference as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RL_ERR_INVALID, RL_ERR_UNSUPPORTED = -1, -3


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


class _Dev:
    """A device buffer of `dtype` holding a host array (rl_device_alloc)."""

    def __init__(self, host, dtype):
        L = _lib()
        self.ctx = L.Context.get(0)
        self.dtype = dtype
        self.dev = ctypes.c_void_p()
        host = np.ascontiguousarray(host, dtype=np.float64)
        L.check(L.lib.rl_device_alloc(self.ctx.handle, max(host.size, 1) * (4 if dtype == 'f32' else 8), ctypes.byref(self.dev)))
        L.check(L.lib.rl_device_upload(self.ctx.handle, self.dev, L.DTYPES[dtype], host.size, L.ptr(host)))

    def __del__(self):
        L = _lib()
        if L.lib is not None and self.dev.value:
            L.lib.rl_device_free(self.ctx.handle, self.dev)
            self.dev = ctypes.c_void_p()


def _sectors(a, a_off, b, b_off, shape, S, scale=None, n_rings=None):
    from rescan_line_sted_amd import quality
    return quality.sector_stats_device(a.ctx, a.dev, a.dtype, a_off, b.dev, b.dtype, b_off, shape, S, scale, n_rings)


def _rings(a, a_off, b, b_off, shape, scale=None, n_rings=None):
    from rescan_line_sted_amd import quality
    return quality.ring_stats_device(a.ctx, a.dev, a.dtype, a_off, b.dev, b.dtype, b_off, shape, scale, n_rings)


@pytest.mark.parametrize('case', [((8, 8), 12), ((37, 50), 6), ((96, 160), 5), ((160, 160), 6)])
def test_parity_with_numpy(case):
    """a and b in ONE f32 buffer at odd element offsets; at 37 x 50 also an f64 truth buffer that three pairs reference under three
    scales; 96 x 160 with S = 5 as f32 against f64."""
    (ny, nx), S = case
    pix = ny * nx
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny * 7 + nx)
    a, b, obj = rr.poisson_pair(rng, ny, nx, *sr.LEVEL[(ny, nx)])
    host = np.zeros(1 + 2 * pix + 2)
    offs = [1, 1 + pix + 2 - (pix % 2)]                     # both odd
    assert all(o % 2 == 1 for o in offs)
    host[offs[0]:offs[0] + pix] = a.ravel()
    host[offs[1]:offs[1] + pix] = b.ravel()
    buf = _Dev(host, 'f32')
    label = '%dx%d S=%d ' % (ny, nx, S)
    if (ny, nx) == (96, 160):
        other = _Dev(np.concatenate([[0.0], b.ravel()]), 'f64')
        got = _sectors(buf, [offs[0]], other, [1], (ny, nx), S)
        assert got.shape == (1, R, S, 5)
        sr.check_cells(got[0], a, b, 1.0, R, S, label + 'f32/f64')
        return
    got = _sectors(buf, [offs[0], offs[1]], buf, [offs[1], offs[0]], (ny, nx), S)
    assert got.shape == (2, R, S, 5)
    sr.check_cells(got[0], a, b, 1.0, R, S, label + 'f32/f32 (a, b)')
    sr.check_cells(got[1], b, a, 1.0, R, S, label + 'f32/f32 (b, a)')
    if (ny, nx) == (37, 50):
        truth = _Dev(np.concatenate([[0.0], obj.ravel()]), 'f64')
        scales = [1.0, a.sum() / obj.sum(), 0.31]
        got = _sectors(buf, [offs[0], offs[1], offs[0]], truth, [1, 1, 1], (ny, nx), S, scales)
        for k, (img, s) in enumerate(zip((a, b, a), scales)):
            sr.check_cells(got[k], img, obj, s, R, S, label + 'f32/f64 truth, scale %.3g' % s)
        more = _sectors(buf, [offs[0]], truth, [1], (ny, nx), S, None, 2 * R + 1)
        sr.check_cells(more[0], a, obj, 1.0, 2 * R + 1, S, label + '37 rings', guard=False)


def test_batch_independence_and_repeatability():
    """70 pairs at 64 x 64 with S = 5 in one call equal the same pairs one at a time, and a second call, bit for bit."""
    n, ny, nx, S = 70, 64, 64, 5
    rng = np.random.default_rng(70)
    imgs = rng.poisson(30.0, size=(n + 1, ny, nx)).astype(np.float64)
    buf = _Dev(imgs, 'f32')
    pix = ny * nx
    a_off = np.arange(n) * pix
    b_off = (np.arange(n) + 1) * pix
    scale = 0.5 + rng.random(n)
    together = _sectors(buf, a_off, buf, b_off, (ny, nx), S, scale)
    again = _sectors(buf, a_off, buf, b_off, (ny, nx), S, scale)
    assert np.array_equal(together, again)
    for k in range(n):
        alone = _sectors(buf, a_off[k:k + 1], buf, b_off[k:k + 1], (ny, nx), S, scale[k:k + 1])
        assert np.array_equal(alone[0], together[k]), k
    sr.check_cells(together[69], imgs[69], imgs[70], scale[69], 32, S, '64x64 S=5 pair 69 of 70', guard=False)


@pytest.mark.parametrize('shape,S,f,sector', sr.GRATINGS)
def test_gratings_land_in_their_sector(shape, S, f, sector):
    ny, nx = shape
    a = _Dev(sr.grating(ny, nx, *f), 'f64')
    zero = _Dev(np.zeros(shape), 'f64')
    sr.check_grating(_sectors(a, [0], zero, [0], shape, S)[0], shape, S, f, sector)


@pytest.mark.parametrize('case', [((37, 50), 6), ((96, 160), 5), ((64, 64), 1)])
def test_sector_sums_give_the_ring_statistics_and_leave_them_alone(case):
    """rl_ring_sector_stats summed over the sectors against rl_ring_stats of the same pairs; and rl_ring_stats before and after a
    sector call on the same context, bit for bit (the tables and the workspace of the two do not interfere)."""
    (ny, nx), S = case
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny + nx + S)
    a, b, _ = rr.poisson_pair(rng, ny, nx)
    buf = _Dev(np.stack([a, b]), 'f32')
    offs = ([0, ny * nx], [ny * nx, 0])
    scale = [0.61, 1.0]
    before = _rings(buf, offs[0], buf, offs[1], (ny, nx), scale)
    sec = _sectors(buf, offs[0], buf, offs[1], (ny, nx), S, scale)
    after = _rings(buf, offs[0], buf, offs[1], (ny, nx), scale)
    assert np.array_equal(before, after)
    for k, (x, y) in enumerate(((a, b), (b, a))):
        assert np.array_equal(sec[k, ..., 0].sum(axis=1), before[k, :, 0])
        allow = sr.bound(x, y, S, scale[k], R).sum(axis=1) + rr.bound(x, y, scale[k], R)
        err = np.abs(sec[k].sum(axis=1)[:, 1:] - before[k, :, 1:]).max(axis=1)
        print('%dx%d S=%d pair %d: max |sum over sectors - ring| / allowance %.3g' % (ny, nx, S, k, float(np.max(err / allow))))
        assert np.all(err <= allow)


# ------------------------------------------------------------------ the Python layer
def _objects():
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {'rings': o['rings'][0].astype(np.float64)}                              # 128 x 128


def _psf_sets():
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    return {'point': [g['1p5x_lr/point_sted_psf'][0]], 'line3': [p[None] for p in g['1p5x_lr/line_sted_psfs'][:, 0]]}


BRIGHT = 1e6
S6 = 6                                                                               # 2 x 3 scan angles: best angle sector 0, worst sector 1


@pytest.fixture(scope='module')
def two_seeds():
    """The `rings` object under the point and the 3-line PSF sets at two seeds, 20 iterations: (tasks, DeviceResults, downloaded
    estimates, objects)."""
    from rescan_line_sted_amd import sweep
    objects, psf_sets = _objects(), _psf_sets()
    tasks = sweep.make_tasks(objects, psf_sets, (3, 4))
    order = sweep.sort_by_group(tasks, objects)
    tasks = [tasks[i] for i in order]
    res = sweep.run_tasks_device(tasks, objects, psf_sets, 20, total_brightness=BRIGHT, dtype='f32')
    return tasks, res, res.download(), objects


def test_score_tasks_with_sectors(two_seeds):
    from rescan_line_sted_amd import quality, sweep
    tasks, res, est, objects = two_seeds
    obj = objects['rings']
    s = BRIGHT / obj.sum()
    sc = sweep.score_tasks(res, tasks, objects, BRIGHT, n_sectors=S6)
    assert sc.shape == (len(tasks), 64, S6, 5) and len(tasks) == 4
    plain = sweep.score_tasks(res, tasks, objects, BRIGHT)
    assert plain.shape == (len(tasks), 64, 5)
    for i in range(len(tasks)):
        # the host route uploads the same values (f32 estimates are exact in float64) and runs the same kernels: the same bits
        assert np.array_equal(sc[i], quality.sector_stats(est[i], obj, S6, scale=s)), i
        sr.check_cells(sc[i], est[i], obj, s, 64, S6, 'score_tasks(n_sectors=6) task %d vs numpy' % i, guard=False)
        summed = quality.rings_from_sectors(sc[i])
        assert np.array_equal(summed[:, 0], plain[i][:, 0])
        allow = sr.bound(est[i], obj, S6, s, 64).sum(axis=1) + rr.bound(est[i], obj, s, 64)
        assert np.all(np.abs(summed[:, 1:] - plain[i][:, 1:]).max(axis=1) <= allow)
    freq, angles, prof = quality.directional_fourier_error(est[0], s * obj, S6)
    assert prof.shape == (64, S6) and np.array_equal(angles, quality.sector_angles(S6)) and np.array_equal(freq, quality.ring_frequencies(64))
    assert np.array_equal(prof, quality.radial_error_from_stats(sc[0], (128, 128)), equal_nan=True)
    # the figure's contrast: the 3-line set's error in its best direction (sector 0) against its worst (sector 1) over the upper
    # half of the rings, beside the point PSF's.  Printed, not asserted: the size of the contrast at this dose is not known.
    for i, (o, p, seed) in enumerate(tasks):
        e = np.nanmean(quality.radial_error_from_stats(sc[i], (128, 128))[32:], axis=0)
        print('%s seed %d: mean error of rings 32..63 by sector %s, worst (sector 1) / best (sector 0) %.3f'
              % (p, seed, ' '.join('%.4g' % x for x in e), e[1] / e[0]))


def test_frc_between_seeds_with_sectors(two_seeds):
    from rescan_line_sted_amd import quality, sweep
    tasks, res, est, _ = two_seeds
    keys, st = sweep.frc_between_seeds(res, tasks, 3, 4, n_sectors=S6)
    assert sorted(keys) == [('rings', 'line3'), ('rings', 'point')] and st.shape == (2, 64, S6, 5)
    for (o, p), cells in zip(keys, st):
        ia, ib = tasks.index((o, p, 3)), tasks.index((o, p, 4))
        sr.check_cells(cells, est[ia], est[ib], 1.0, 64, S6, 'frc_between_seeds(n_sectors=6) %s vs numpy' % p, guard=False)
        by_angle = quality.frc_resolution_by_angle(cells)
        assert by_angle.shape == (S6,) and np.all(by_angle > 0)
        print('%s: FRC 1/7 period in pixels by angle %s' % (p, np.round(by_angle, 2).tolist()))
    assert sweep.frc_between_seeds(res, tasks, 3, 4)[1].shape == (2, 64, 5)


def test_scored_sweep_with_sectors():
    """figure_2_sweep(scores=True, n_sectors=6): the estimates of the unscored sweep, and scores equal to score_tasks of them."""
    from rescan_line_sted_amd import sweep
    objects, psf_sets = _objects(), _psf_sets()
    kw = dict(seeds=(0, 7), iterations=4, total_brightness=BRIGHT, dtype='f32')
    tasks0, est0 = sweep.figure_2_sweep(objects, psf_sets, **kw)
    tasks, est, scores = sweep.figure_2_sweep(objects, psf_sets, scores=True, n_sectors=S6, **kw)
    assert tasks == tasks0 and len(tasks) == 4
    assert np.array_equal(est, est0)
    assert np.asarray(scores).shape == (4, 64, S6, 5)
    res = sweep.DeviceResults.from_host(list(est), 'f32')                         # (f32 estimates: exact in float64 and back)
    again = sweep.score_tasks(res, tasks, objects, BRIGHT, n_sectors=S6)
    assert np.array_equal(scores, again)
    t16, _, s16 = sweep.figure_2_sweep(objects, psf_sets, seeds=(0,), iterations=2, total_brightness=BRIGHT, scores=True, n_rings=16,
                                       n_sectors=2)
    assert np.asarray(s16).shape == (len(t16), 16, 2, 5)


# ------------------------------------------------------------------ error codes
def test_error_codes():
    L = _lib()
    buf = _Dev(np.ones(64), 'f32')
    out = np.zeros(4 * 64 * 5)
    off = (ctypes.c_int64 * 1)(0)
    neg = (ctypes.c_int64 * 1)(-1)
    h, d = buf.ctx.handle, buf.dev

    def call(ctx=h, a=d, ao=off, b=d, bo=off, n=1, ny=8, nx=8, R=4, S=3, o=out, adt=0, bdt=0):
        return L.lib.rl_ring_sector_stats(ctx, a, adt, ao, b, bdt, bo, None, n, ny, nx, R, S, L.ptr(o) if o is not None else None)
    assert call() == 0 and list(out[:5]) == [1.0, 64.0 ** 2, 64.0 ** 2, 64.0 ** 2, 0.0]      # cell (0, 0) is the DC bin
    assert np.all(out[5:15] == 0.0)                                                          # ring 0 has no other cell
    assert call(S=64) == 0 and call(S=1) == 0
    assert call(S=0) == RL_ERR_INVALID and call(S=-1) == RL_ERR_INVALID
    assert call(S=65) == RL_ERR_UNSUPPORTED
    assert b'64 sectors' in L.lib.rl_last_error()
    for kw in (dict(ctx=None), dict(a=None), dict(b=None), dict(ao=None), dict(bo=None), dict(o=None), dict(n=0), dict(ny=1), dict(nx=1),
               dict(R=0), dict(adt=7), dict(bdt=-1), dict(ao=neg)):
        assert call(**kw) == RL_ERR_INVALID, kw
    assert call(ny=4097) == RL_ERR_UNSUPPORTED and call(nx=4097) == RL_ERR_UNSUPPORTED
    assert b'4096' in L.lib.rl_last_error()
    assert call(R=16385) == RL_ERR_UNSUPPORTED
