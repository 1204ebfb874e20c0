"""The ring statistics on the MI355X (include/rlsted.h rl_ring_stats): parity with numpy (tests/ring_reference.py) under the derived
bound, batch independence bit for bit, the Python layer on a sweep's device-resident estimates (FRC between seeds, scores against the
true object, the existing fourier_error), the scored sweep, and the error codes."""
import ctypes
import os

import numpy as np
import pytest

import ring_reference as rr
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


def _stats(a, a_off, b, b_off, shape, scale=None, n_rings=None):
    from rescan_line_sted_amd import quality
    return quality.ring_stats_device(a.ctx, a.dev, a.dtype, a_off, b.dev, b.dtype, b_off, shape, scale, n_rings)


def _check(got, a, b, scale, R, label, guard=True):
    """One pair's fields against ring_reference under its bound (printed first).  guard: the bound is at most 1e-9 of field 1 in
    every ring, so it cannot swallow a wrong answer."""
    want, bound = rr.ring_stats(a, b, scale, R), rr.bound(a, b, scale, R)
    err = np.abs(got[:, 1:] - want[:, 1:]).max(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s: max err / bound %.3g, max bound / field1 %.3g' % (label, float(np.max(err / bound)), float(np.nanmax(bound / want[:, 1]))))
    assert np.array_equal(got[:, 0], want[:, 0]), label
    if guard:
        assert np.all(bound <= 1e-9 * want[:, 1]), (label, float(np.max(bound / want[:, 1])))
    assert np.all(err <= bound), (label, float(np.max(err / bound)))


# (mean, offset) of the Poisson images per shape: dim enough that the bound stays below 1e-9 of every ring's power -- the bound
# over a noise ring's power is about 16 L u sqrt(sum of the image), L = ring_reference.chain_length
LEVEL = {(8, 8): (200.0, 20.0), (37, 50): (100.0, 10.0), (96, 160): (5.0, 1.0), (128, 128): (5.0, 1.0), (160, 160): (5.0, 1.0),
         (512, 512): (0.05, 0.01)}


@pytest.mark.parametrize('shape', sorted(LEVEL))
def test_parity_with_numpy(shape):
    """a and b in ONE f32 buffer at odd element offsets (the two-seeds case); at 37 x 50 also an f64 truth buffer that three pairs
    reference under three scales."""
    ny, nx = shape
    pix = ny * nx
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny * 7 + nx)
    a, b, obj = rr.poisson_pair(rng, ny, nx, *LEVEL[shape])
    host = np.zeros(1 + 2 * pix + 2)
    offs = [1, 1 + pix + 2 - (pix % 2)]                     # both odd
    assert all(o % 2 == 1 for o in offs)
    host[offs[0]:offs[0] + pix] = a.ravel()
    host[offs[1]:offs[1] + pix] = b.ravel()
    buf = _Dev(host, 'f32')
    got = _stats(buf, [offs[0], offs[1]], buf, [offs[1], offs[0]], shape)
    assert got.shape == (2, R, 5)
    _check(got[0], a, b, 1.0, R, '%dx%d f32/f32 (a, b)' % shape)
    _check(got[1], b, a, 1.0, R, '%dx%d f32/f32 (b, a)' % shape)
    if shape == (37, 50):
        truth = _Dev(np.concatenate([[0.0], obj.ravel()]), 'f64')
        scales = [1.0, a.sum() / obj.sum(), 0.31]
        got = _stats(buf, [offs[0], offs[1], offs[0]], truth, [1, 1, 1], shape, scales)
        for k, (img, s) in enumerate(zip((a, b, a), scales)):
            _check(got[k], img, obj, s, R, '37x50 f32/f64 truth, scale %.3g' % s)
        _check(_stats(buf, [offs[0]], truth, [1], shape, None, 2 * R + 1)[0], a, obj, 1.0, 2 * R + 1, '37x50, 37 rings', guard=False)


def test_batch_independence_and_repeatability():
    """70 pairs at 64 x 64 in one call equal the same pairs one at a time, and a second call, bit for bit."""
    n, ny, nx = 70, 64, 64
    rng = np.random.default_rng(70)
    imgs = rng.poisson(30.0, size=(n + 1, ny, nx)).astype(np.float64)
    buf = _Dev(imgs, 'f32')
    pix = ny * nx
    a_off = np.arange(n) * pix
    b_off = (np.arange(n) + 1) * pix
    scale = 0.5 + rng.random(n)
    together = _stats(buf, a_off, buf, b_off, (ny, nx), scale)
    again = _stats(buf, a_off, buf, b_off, (ny, nx), scale)
    assert np.array_equal(together, again)
    for k in range(n):
        alone = _stats(buf, a_off[k:k + 1], buf, b_off[k:k + 1], (ny, nx), scale[k:k + 1])
        assert np.array_equal(alone[0], together[k]), k
    _check(together[69], imgs[69], imgs[70], scale[69], 32, '64x64 pair 69 of 70')


# ------------------------------------------------------------------ the Python layer
def _objects():
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {k: o[k][0].astype(np.float64) for k in ('rings', 'cat')}             # 128 x 128 and 160 x 160


def _psf_sets():
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    return {'point': [g['1p5x_lr/point_sted_psf'][0]], 'line3': [p[None] for p in g['1p5x_lr/line_sted_psfs'][:, 0]]}


BRIGHT = 1e6


@pytest.fixture(scope='module')
def two_seeds():
    """The `rings` object simulated at two seeds, 20 iterations: (tasks, DeviceResults, downloaded estimates)."""
    from rescan_line_sted_amd import sweep
    objects, psf_sets = {'rings': _objects()['rings']}, {'point': _psf_sets()['point']}
    tasks = sweep.make_tasks(objects, psf_sets, (3, 4))
    res = sweep.run_tasks_device(tasks, objects, psf_sets, 20, total_brightness=BRIGHT, dtype='f32')
    return tasks, res, res.download(), objects


def test_frc_between_seeds_on_device_results(two_seeds):
    from rescan_line_sted_amd import quality, sweep
    tasks, res, est, _ = two_seeds
    keys, st = sweep.frc_between_seeds(res, tasks, 3, 4)
    assert keys == [('rings', 'point')] and st.shape == (1, 64, 5)
    ia, ib = tasks.index(('rings', 'point', 3)), tasks.index(('rings', 'point', 4))
    assert not np.array_equal(est[ia], est[ib])
    _check(st[0], est[ia], est[ib], 1.0, 64, 'frc_between_seeds vs numpy', guard=False)
    # the host-array route uploads the same values (f32 estimates are exact in float64) and runs the same kernels: same sums
    host = quality.ring_stats(est[ia], est[ib])
    _check(host, est[ia], est[ib], 1.0, 64, 'quality.ring_stats vs numpy', guard=False)
    assert np.array_equal(host, st[0])
    freq, curve = quality.frc(est[ia], est[ib])
    assert np.array_equal(curve, quality.frc_from_stats(st[0]), equal_nan=True)
    assert curve[0] > 0.99                                                       # two realisations of one object agree at low frequency
    assert np.isfinite(quality.frc_resolution(freq, curve)) or np.all(curve >= 1 / 7)
    with pytest.raises(ValueError):
        sweep.frc_between_seeds(res, tasks, 3, 99)


def test_score_tasks_against_fourier_error(two_seeds):
    """Field 4 of score_tasks is the ring-binned square of the existing quality.fourier_error * ny nx (ref2:353-355) of the estimate
    against the object at the simulated brightness; radial_fourier_error is its ring RMS."""
    from rescan_line_sted_amd import quality, sweep
    tasks, res, est, objects = two_seeds
    sc = sweep.score_tasks(res, tasks, objects, BRIGHT)
    assert sc.shape == (2, 64, 5)
    obj = objects['rings']
    s = BRIGHT / obj.sum()
    table = rr.ring_table(128, 128)
    for i in range(2):
        _check(sc[i], est[i], obj, s, 64, 'score_tasks task %d vs numpy' % i, guard=False)
        d = est[i] - s * obj
        fe = np.fft.ifftshift(quality.fourier_error(est[i], s * obj)) * (128 * 128)        # |fft2(d)| by the existing kernels
        binned = np.bincount(table.ravel(), weights=(fe ** 2).ravel(), minlength=65)[:64]
        # fourier_error's own error per value: a float64 DFT of d summed term by term, at most gamma_L ||d||_1 (L as ours, generously)
        e_fe = rr.gamma(rr.chain_length(128, 128)) * np.abs(d).sum()
        own = np.bincount(table.ravel(), weights=(2 * e_fe * fe + e_fe ** 2).ravel(), minlength=65)[:64] + rr.gamma(sc[i][:, 0]) * binned
        err = np.abs(sc[i][:, 4] - binned)
        print('task %d: field 4 vs binned fourier_error^2: max err / allowance %.3g' % (i, float(np.max(err / (rr.bound(est[i], obj, s) + own)))))
        assert np.all(err <= rr.bound(est[i], obj, s) + own)
        freq, prof = quality.radial_fourier_error(est[i], s * obj)
        assert np.array_equal(freq, quality.ring_frequencies(64))
        # the same values through the host route (s * obj is the one rounding the device makes too): the same bits, and so the
        # profile squared back to field 4 meets the binned fourier_error^2 under the same allowance (+ its own 8 roundings)
        assert np.array_equal(prof, quality.radial_error_from_stats(sc[i], (128, 128)))
        back = (prof * (128 * 128)) ** 2 * sc[i][:, 0]
        assert np.all(np.abs(back - binned) <= rr.bound(est[i], obj, s) + own + 8 * rr.U * binned)


def test_device_results_ring_stats_arguments(two_seeds):
    from rescan_line_sted_amd import sweep
    tasks, res, est, objects = two_seeds
    mixed = sweep.DeviceResults.from_host([np.ones((8, 8)), np.ones((8, 10))], 'f32')
    with pytest.raises(ValueError):
        mixed.ring_stats([0, 1], b_idx=[0, 1])
    with pytest.raises(ValueError):
        res.ring_stats([0], truth=mixed, truth_index=[0])
    with pytest.raises(ValueError):
        res.ring_stats([0])
    truth = sweep.DeviceResults.from_host([objects['rings']], 'f64')
    one = res.ring_stats([0, 1], truth=truth, scale=2.0)                          # one truth for every pair, one scale
    _check(one[1], est[1], objects['rings'], 2.0, 64, 'one truth, scalar scale', guard=False)


def test_scored_sweep_matches_unscored_sweep_and_score_tasks():
    """2 objects (128 x 128, 160 x 160) x 2 PSF sets x 2 seeds: the estimates of scores=True are those of scores=False, and the scores
    are score_tasks of them."""
    from rescan_line_sted_amd import sweep
    objects, psf_sets = _objects(), _psf_sets()
    tasks0, est0 = sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 7), iterations=4, total_brightness=BRIGHT, dtype='f32')
    tasks, est, scores = sweep.figure_2_sweep(objects, psf_sets, seeds=(0, 7), iterations=4, total_brightness=BRIGHT, dtype='f32', scores=True)
    assert tasks == tasks0 and len(tasks) == 8
    assert all(np.array_equal(a, b) for a, b in zip(est, est0))
    assert [s.shape for s in scores] == [(min(e.shape) // 2, 5) for e in est]
    res = sweep.DeviceResults.from_host(est, 'f32')                               # (f32 estimates: exact in float64 and back)
    again = sweep.score_tasks(res, tasks, objects, BRIGHT)
    assert all(np.array_equal(a, b) for a, b in zip(scores, again))
    o, p, _ = tasks[5]
    _check(scores[5], est[5], objects[o], BRIGHT / objects[o].sum(), min(est[5].shape) // 2, 'sweep score of task 5', guard=False)
    t32, _, s32 = sweep.figure_2_sweep(objects, psf_sets, seeds=(0,), iterations=2, total_brightness=BRIGHT, scores=True, n_rings=32)
    assert np.asarray(s32).shape == (len(t32), 32, 5)


def test_scored_sweep_through_the_device_gather_world_1(tmp_path):
    """The device-gather route (sharding.RcclComm, world size 1): scored on the device before rl_comm_gather_device, the answers of the
    route without a communicator."""
    from rescan_line_sted_amd import sharding, sweep
    objects, psf_sets = _objects(), _psf_sets()
    kw = dict(seeds=(0, 7), iterations=4, total_brightness=BRIGHT, dtype='f32', scores=True)
    tasks, est, scores = sweep.figure_2_sweep(objects, psf_sets, **kw)
    comm = sharding.RcclComm(0, 1, device=0, path=str(tmp_path / 'id'))
    tasks_c, est_c, scores_c = sweep.figure_2_sweep(objects, psf_sets, comm=comm, **kw)
    comm.close()
    assert tasks_c == tasks and all(np.array_equal(a, b) for a, b in zip(est_c, est))
    assert all(np.array_equal(a, b) for a, b in zip(scores_c, scores))
    sweep.clear_plans()


# ------------------------------------------------------------------ error codes
def test_error_codes():
    L = _lib()
    buf = _Dev(np.ones(64), 'f32')
    out = np.zeros(4 * 5)
    off = (ctypes.c_int64 * 1)(0)
    h, d = buf.ctx.handle, buf.dev

    def call(ctx=h, a=d, ao=off, b=d, bo=off, n=1, ny=8, nx=8, R=4, o=out, adt=0, bdt=0):
        return L.lib.rl_ring_stats(ctx, a, adt, ao, b, bdt, bo, None, n, ny, nx, R, L.ptr(o) if o is not None else None)
    assert call() == 0 and out[0] == 1.0 and out[1] == 64.0 ** 2                  # ring 0 is the DC bin: |sum of ones|^2
    for kw in (dict(ctx=None), dict(a=None), dict(b=None), dict(ao=None), dict(bo=None), dict(o=None), dict(n=0), dict(ny=1), dict(nx=1),
               dict(R=0), dict(adt=7)):
        assert call(**kw) == RL_ERR_INVALID, kw
    assert call(ny=4097) == RL_ERR_UNSUPPORTED and call(nx=4097) == RL_ERR_UNSUPPORTED
    assert b'4096' in L.lib.rl_last_error()
    assert L.lib.rl_ring_count(160, 128) == 64
