"""The ensemble statistics on the MI355X (include/rlsted.h rl_ensemble_stats): parity of the maps and the pixel sums with numpy long
double under the derived bound (tests/ensemble_reference.py), run-to-run and group independence bit for bit, the cancellation case
no one-pass formula survives, the launch chunking, the Python layer on a sweep's device-resident estimates -- ensemble_tasks, the
spectral split from the ring entry points, the curves over the iteration count, the sharded sweep's option -- and the error codes."""
import ctypes
import os

import numpy as np
import pytest

import ensemble_reference as er
import ring_reference as rr
import sector_reference as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RL_ERR_INVALID = -1
SIZES = (1, 2, 3, 16, 17)


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
        self.size = host.size
        L.check(L.lib.rl_device_alloc(self.ctx.handle, max(host.size, 1) * (4 if dtype == 'f32' else 8), ctypes.byref(self.dev)))
        L.check(L.lib.rl_device_upload(self.ctx.handle, self.dev, L.DTYPES[dtype], host.size, L.ptr(host)))

    def download(self):
        L = _lib()
        out = np.empty(self.size)
        L.check(L.lib.rl_device_download(self.ctx.handle, self.dev, L.DTYPES[self.dtype], self.size, L.ptr(out)))
        return out

    def __del__(self):
        L = _lib()
        if L.lib is not None and self.dev.value:
            L.lib.rl_device_free(self.ctx.handle, self.dev)
            self.dev = ctypes.c_void_p()


class _OnDevice:
    """An ensemble_reference.Case uploaded: the member buffer and the truth buffer."""

    def __init__(self, case):
        self.case = case
        self.src = _Dev(case.buf, case.dtype)                    # (the case's values are exact in its dtype: the upload rounds nothing)
        self.truth = _Dev(case.truth_buf, case.truth_dtype)

    def run(self, groups=None, truth=True, maps=True):
        """(mean [G][N], var [G][N], out [G][6]) of the groups `groups` (indices into the case's; None: all)."""
        from rescan_line_sted_amd import quality
        c = self.case
        gs = list(range(len(c.sizes)) if groups is None else groups)
        mean = _Dev(np.full(len(gs) * c.N, np.nan), 'f64') if maps else None
        var = _Dev(np.full(len(gs) * c.N, np.nan), 'f64') if maps else None
        t = (self.truth.dev, c.truth_dtype, [c.truth_off[g] for g in gs], [c.scale[g] for g in gs]) if truth else None
        out = quality.ensemble_stats_device(self.src.ctx, self.src.dev, c.dtype, [c.offsets[g] for g in gs], c.N, truth=t,
                                            mean_dev=mean.dev if maps else None, var_dev=var.dev if maps else None)
        assert out.shape == (len(gs), 6)
        if not maps:
            return None, None, out
        return mean.download().reshape(len(gs), c.N), var.download().reshape(len(gs), c.N), out


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('shape', [(37, 50), (96, 160), (128, 128), (8197,)])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_parity_with_long_double(dtype, shape):
    """Groups of 1, 2, 3, 16 and 17 members in one call, the images at odd and even element offsets of one buffer (both load paths),
    one image listed in two groups, a truth of the other type at 96 x 160; every group's maps and sums under the derived bound; then
    the call without a truth and the call without maps."""
    N = int(np.prod(shape))
    rng = np.random.default_rng(N + (dtype == 'f64'))
    case = er.Case(rng, dtype, N, SIZES, shift=1, truth_dtype='f32' if shape == (96, 160) else 'f64')
    assert any(o % 2 == 1 for offs in case.offsets for o in offs) and any(o % 4 == 0 for offs in case.offsets for o in offs)
    dev = _OnDevice(case)
    mean, var, out = dev.run()
    assert not np.isnan(mean).any() and not np.isnan(var).any()                     # every pixel of every map was written
    for g, n in enumerate(SIZES):
        case.reference(g).check(out[g], mean[g], var[g], '%s %s n=%d' % (dtype, 'x'.join(map(str, shape)), n))
    assert np.all(var[0] == 0.0) and out[0, 2] == 0.0                               # n = 1: exactly 0
    m2, v2, o2 = dev.run(truth=False)
    assert np.array_equal(o2[:, :3], out[:, :3]) and np.all(o2[:, 3:] == 0.0)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    assert np.array_equal(dev.run(maps=False)[2], out)


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_repeatability_and_group_independence(dtype):
    """A second call, every group alone and the groups in reverse order give the bits of the first call (flat 8197: two workgroups
    per group, a partial last vector)."""
    case = er.Case(np.random.default_rng(8197), dtype, 8197, SIZES, shift=1)
    dev = _OnDevice(case)
    mean, var, out = dev.run()
    again = dev.run()
    assert np.array_equal(again[2], out) and np.array_equal(again[0], mean) and np.array_equal(again[1], var)
    for g in range(len(SIZES)):
        m1, v1, o1 = dev.run([g])
        assert np.array_equal(o1[0], out[g]) and np.array_equal(m1[0], mean[g]) and np.array_equal(v1[0], var[g]), g
    rev = dev.run([4, 3, 2, 1, 0])
    assert np.array_equal(rev[2][::-1], out) and np.array_equal(rev[0][::-1], mean)


def test_cancellation_needs_the_second_pass():
    """f64 values 1e8 + N(0, 1), n = 16: the derived bound is below 1e-9 of ss, and the kernel meets it."""
    case = er.Case(np.random.default_rng(16), 'f64', 128 * 128, (16,), shift=1, cancel=True)
    ref = case.reference(0)
    ss = ref.ss.astype(np.float64)
    assert np.all(ref.e_ss < 1e-9 * ss)
    sums, bnd = ref.sums()
    assert bnd[2] < 1e-9 * float(sums[2])
    mean, var, out = _OnDevice(case).run()
    ref.check(out[0], mean[0], var[0], 'cancellation f64 128x128 n=16')
    x = case.members(0)
    one_pass = (x * x).sum(axis=0) - 16 * x.mean(axis=0) ** 2
    print('relative error of ss: the kernel %.3g, one pass in numpy %.3g'
          % (float(np.max(np.abs(var[0] * 15 - ss) / ss)), float(np.max(np.abs(one_pass - ss) / ss))))
    assert float(np.max(np.abs(var[0] * 15 - ss) / ss)) < 1e-12


def test_more_groups_than_one_launch_holds():
    """70 000 groups of two 3-pixel images (image i and i + 1 of an f32 buffer): the second launch starts at group 65 535.  One
    thread sums a group's single vector, so numpy's float64 in the same order gives the very bits."""
    G, N = 70000, 3
    rng = np.random.default_rng(70000)
    host = rng.poisson(50.0, size=(G + 1) * N).astype(np.float64) + 0.5
    truth = rng.random(N) * 50.0
    src, tr = _Dev(host, 'f32'), _Dev(truth, 'f64')
    from rescan_line_sted_amd import quality
    mean = _Dev(np.full(G * N, np.nan), 'f64')
    out = quality.ensemble_stats_device(src.ctx, src.dev, 'f32', [[i * N, (i + 1) * N] for i in range(G)], N,
                                        truth=(tr.dev, 'f64', np.zeros(G, dtype=np.int64), None), mean_dev=mean.dev)
    x = host.reshape(G + 1, N)
    m = ((0.0 + x[:-1]) + x[1:]) / 2.0
    d0, d1 = x[:-1] - m, x[1:] - m
    v = ((d0 * d0) + (d1 * d1)) / 1.0
    b = m - truth
    e0, e1 = x[:-1] - truth, x[1:] - truth
    mse = ((e0 * e0) + (e1 * e1)) / 2.0

    def seq(a):
        return ((0.0 + a[:, 0]) + a[:, 1]) + a[:, 2]
    want = np.stack([np.full(G, 2.0), seq(m), seq(v), seq(b * b), seq(mse), np.full(G, seq((truth * truth)[None])[0])], axis=1)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5].tolist()
    assert np.array_equal(mean.download().reshape(G, N), m)


def test_host_convenience_goes_through_the_same_entry_point():
    from rescan_line_sted_amd import quality
    rng = np.random.default_rng(5)
    stacks = [rng.poisson(40.0, size=(n, 37, 50)).astype(np.float64) for n in (3, 1, 5)]
    truth = 40.0 * (0.8 + 0.4 * rng.random((37, 50)))
    mean, var, sc = quality.ensemble_stats(stacks, truth=truth, scale=[1.0, 0.5, 2.0])
    assert mean.shape == var.shape == (3, 37, 50) and sc.shape == (3, 6)
    for g, (s, scale) in enumerate(zip(stacks, (1.0, 0.5, 2.0))):
        er.Reference(s.reshape(s.shape[0], -1), truth, scale).check(sc[g], mean[g], var[g], 'ensemble_stats group %d' % g)
    m1, v1, s1 = quality.ensemble_stats(stacks[2], truth=truth, scale=2.0)
    assert m1.shape == (37, 50) and np.array_equal(m1, mean[2]) and np.array_equal(v1, var[2]) and np.array_equal(s1, sc[2])
    m0, v0, s0 = quality.ensemble_stats(stacks[0])
    assert np.array_equal(m0, mean[0]) and np.all(s0[3:] == 0.0) and np.array_equal(s0[:3], sc[0, :3])


# ------------------------------------------------------------------ the Python layer on a sweep
def _objects(names=('rings', 'lines')):
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {n: o[n][0].astype(np.float64) for n in names}                            # 128 x 128; 'cat' is 160 x 160


def _psf_sets():
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    return {'point': [g['1p5x_lr/point_sted_psf'][0]], 'line2': [p[None] for p in g['1p5x_lr/line_sted_psfs'][:2, 0]]}


BRIGHT = 1e6
SEEDS = (3, 4, 5, 6)
S6 = 6


@pytest.fixture(scope='module')
def small_sweep():
    """Two 128 x 128 objects under the point and a 2-view line PSF set at four seeds, 8 iterations: (tasks, DeviceResults, downloaded
    estimates, objects, psf sets).  Nothing here is changed by the tests."""
    from rescan_line_sted_amd import sweep
    objects, psf_sets = _objects(), _psf_sets()
    tasks = sweep.make_tasks(objects, psf_sets, SEEDS)
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    res = sweep.run_tasks_device(tasks, objects, psf_sets, 8, total_brightness=BRIGHT, dtype='f32')
    return tasks, res, res.download(), objects, psf_sets


def _check_against_numpy(keys, counts, means, variances, scalars, tasks, est, objects, label):
    from rescan_line_sted_amd import sweep
    k2, members = sweep.ensemble_keys(tasks)
    assert keys == k2 and list(counts) == [len(m) for m in members]
    mean_maps, var_maps = means.download(), variances.download()
    for k, ((o, p), mem) in enumerate(zip(keys, members)):
        obj = objects[o]
        assert mean_maps[k].shape == obj.shape
        ref = er.Reference(np.stack([est[i].ravel() for i in mem]), obj, BRIGHT / obj.sum())
        ref.check(scalars[k], mean_maps[k], var_maps[k], '%s %s/%s' % (label, o, p))


def test_ensemble_tasks_against_numpy(small_sweep):
    from rescan_line_sted_amd import sweep
    tasks, res, est, objects, _ = small_sweep
    keys, counts, means, variances, scalars = sweep.ensemble_tasks(res, tasks, objects, BRIGHT)
    assert len(keys) == 4 and list(counts) == [4] * 4 and scalars.shape == (4, 6)
    assert means.dtype == variances.dtype == 'f64' and means.ctx.device == res.ctx.device
    _check_against_numpy(keys, counts, means, variances, scalars, tasks, est, objects, 'ensemble_tasks')
    k0, c0, m0, v0, s0 = sweep.ensemble_tasks(res, tasks, objects, BRIGHT, maps=False)
    assert m0 is None and v0 is None and k0 == keys and np.array_equal(s0, scalars)
    # DeviceResults.ensemble on two of the keys, no truth
    _, members = sweep.ensemble_keys(tasks)
    m2, v2, s2 = res.ensemble([members[2], members[0]])
    assert np.array_equal(s2[:, :3], scalars[[2, 0], :3]) and np.all(s2[:, 3:] == 0.0)
    assert np.array_equal(m2.download()[1], means.download()[0])
    for b in (means, variances, m2, v2):
        b.free()


def test_ensemble_tasks_with_two_shapes():
    """160 x 160 and 128 x 128 objects interleave in key order: one call per shape, the maps of key k still image k."""
    from rescan_line_sted_amd import sweep
    objects = _objects(('cat', 'rings', 'lines'))
    psf_sets = {'point': _psf_sets()['point']}
    tasks = sweep.make_tasks(objects, psf_sets, (1, 2))                              # cat, lines, rings per seed
    res = sweep.run_tasks_device(tasks, objects, psf_sets, 2, total_brightness=BRIGHT, dtype='f32')
    keys, counts, means, variances, scalars = sweep.ensemble_tasks(res, tasks, objects, BRIGHT)
    assert [k[0] for k in keys] == ['cat', 'lines', 'rings'] and means.shapes == [(160, 160), (128, 128), (128, 128)]
    _check_against_numpy(keys, counts, means, variances, scalars, tasks, res.download(), objects, 'two shapes')
    with pytest.raises(ValueError):
        res.ensemble([[0, 1]])                                                       # cat and lines in one group
    for b in (means, variances, res):
        b.free()


@pytest.mark.parametrize('n_sectors', [None, S6])
def test_spectral_identity(small_sweep, n_sectors):
    """Per ring and per (ring, sector) cell: the mean over the seeds of field 4 (member, truth) = bias power + (n - 1) / n variance
    power -- |X_m - T|^2 averaged over m splits exactly into |mean - T|^2 and the spread about the mean, bin by bin.  The tolerance
    is the sum of the bounds of the ring statistics on the two sides: the mean over m of bound(member, truth) on the left;
    bound(mean, truth) + 1 / n sum_m bound(member, mean) on the right."""
    from rescan_line_sted_amd import quality, sweep
    tasks, res, est, objects, _ = small_sweep
    keys, counts, spec, mean_stats = sweep.bias_variance_spectrum(res, tasks, objects, BRIGHT, n_sectors=n_sectors)
    cells = (64,) if n_sectors is None else (64, n_sectors)
    assert np.asarray(spec).shape == (4,) + cells + (3,) and np.asarray(mean_stats).shape == (4,) + cells + (5,)
    scores = sweep.score_tasks(res, tasks, objects, BRIGHT, n_sectors=n_sectors)
    _, members = sweep.ensemble_keys(tasks)

    def bound(a, b, s):
        return rr.bound(a, b, s, 64) if n_sectors is None else sr.bound(a, b, n_sectors, s, 64)
    for k, ((o, p), mem) in enumerate(zip(keys, members)):
        n = len(mem)
        obj, s = objects[o], BRIGHT / objects[o].sum()
        mean_img = np.mean([est[i] for i in mem], axis=0)
        left = sum(scores[i][..., 4] for i in mem) / n
        right = spec[k][..., 1] + (n - 1) / n * spec[k][..., 2]
        allow = sum(bound(est[i], obj, s) for i in mem) / n + bound(mean_img, obj, s) + sum(bound(est[i], mean_img, 1.0) for i in mem) / n
        assert np.array_equal(spec[k][..., 0], scores[mem[0]][..., 0])
        err = np.abs(left - right)
        print('%s/%s sectors %s: max |mean field 4 - (bias + (n-1)/n variance)| / allowance %.3g' % (o, p, n_sectors, float(np.max(err / np.where(allow > 0, allow, 1.0)))))   # (an empty cell: 0 against 0)
        assert np.all(err <= allow)
        b_rms, v_rms = quality.spectral_bias_variance_rms(spec[k], obj.shape)
        ssnr = quality.ssnr_from(mean_stats[k], spec[k], n)
        assert b_rms.shape == v_rms.shape == ssnr.shape == cells
        if n_sectors is None:
            print('%s/%s: bias RMS rings 1, 16, 48: %s; noise RMS: %s; SSNR: %s' % (o, p, b_rms[[1, 16, 48]], v_rms[[1, 16, 48]], ssnr[[1, 16, 48]]))


def test_bias_variance_vs_iterations(small_sweep):
    """Every K: mse = b2 + (n - 1) / n var in the reported sums, under the bound of that K's estimates, and the row is what
    ensemble_tasks gives for a sweep of K iterations, bit for bit.  The curves are printed, not judged: which way bias^2 and the
    variance move with K is a property of the data."""
    from rescan_line_sted_amd import sweep
    tasks, _, _, objects, psf_sets = small_sweep
    ks = [1, 4, 16]
    keys, out = sweep.bias_variance_vs_iterations(objects, psf_sets, SEEDS, ks, total_brightness=BRIGHT)
    k2, members = sweep.ensemble_keys(tasks)
    assert keys == k2 and out.shape == (3, 4, 6) and np.all(out[:, :, 0] == 4)
    for j, K in enumerate(ks):
        res = sweep.run_tasks_device(tasks, objects, psf_sets, K, total_brightness=BRIGHT, dtype='f32')
        direct = sweep.ensemble_tasks(res, tasks, objects, BRIGHT, maps=False)[4]
        est = res.download()
        res.free()
        assert np.array_equal(out[j], direct), K
        for k, ((o, p), mem) in enumerate(zip(keys, members)):
            ref = er.Reference(np.stack([est[i].ravel() for i in mem]), objects[o], BRIGHT / objects[o].sum())
            ref.check(out[j, k], label='K=%d %s/%s' % (K, o, p))                     # (asserts the identity under the bound as well)
    for k, (o, p) in enumerate(keys):
        print('%s/%s  K %s: sum bias^2 %s, sum variance %s, sum mse %s' % (o, p, ks, out[:, k, 3], out[:, k, 2], out[:, k, 4]))


def test_sweep_with_ensemble_returns_the_same_estimates():
    from rescan_line_sted_amd import sweep
    objects, psf_sets = _objects(), _psf_sets()
    kw = dict(seeds=(0, 7, 9), iterations=4, total_brightness=BRIGHT, dtype='f32')
    tasks0, est0 = sweep.figure_2_sweep(objects, psf_sets, **kw)
    tasks, est, (keys, scalars) = sweep.figure_2_sweep(objects, psf_sets, ensemble=True, **kw)
    assert tasks == tasks0 and np.array_equal(est, est0)
    assert sorted(keys) == sorted({(o, p) for o, p, _ in tasks}) and scalars.shape == (4, 6) and np.all(scalars[:, 0] == 3)
    res = sweep.DeviceResults.from_host(list(est), 'f32')                         # (f32 estimates: exact in float64 and back)
    k2, _, _, _, again = sweep.ensemble_tasks(res, tasks, objects, BRIGHT, maps=False)
    res.free()
    at = {k: j for j, k in enumerate(k2)}
    assert np.array_equal(scalars, again[[at[k] for k in keys]])
    t3, e3, s3, ens3 = sweep.figure_2_sweep(objects, psf_sets, scores=True, ensemble=True, **kw)
    assert np.array_equal(e3, est0) and np.asarray(s3).shape == (12, 64, 5) and np.array_equal(ens3[1], scalars) and ens3[0] == keys


# ------------------------------------------------------------------ error codes
def test_error_codes():
    L = _lib()
    src = _Dev(np.arange(64, dtype=np.float64), 'f32')
    maps = _Dev(np.zeros(64), 'f64')
    out = np.full(2 * 6, np.nan)
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    off = (i64 * 3)(0, 16, 32)
    gp = (i32 * 3)(0, 2, 3)
    toff = (i64 * 2)(48, 48)
    h, d = src.ctx.handle, src.dev

    def call(ctx=h, s=d, sdt=0, mo=off, g=gp, G=2, t=None, tdt=0, to=None, n=16, mean=None, var=None, o=out):
        return L.lib.rl_ensemble_stats(ctx, s, sdt, mo, g, G, t, tdt, to, None, n, mean, var, L.ptr(o) if o is not None else None)
    assert call() == 0
    assert list(out[:3]) == [2.0, sum(range(8, 24)), 16 * 128.0] and list(out[6:9]) == [1.0, sum(range(32, 48)), 0.0]
    assert np.all(out[[3, 4, 5, 9, 10, 11]] == 0.0)
    assert call(t=d, to=toff) == 0 and out[5] == float(sum(x * x for x in range(48, 64)))
    assert call(mean=maps.dev, var=maps.dev.value + 32 * 8) == 0
    assert list(maps.download()[:3]) == [8.0, 9.0, 10.0]
    for kw in (dict(ctx=None), dict(s=None), dict(mo=None), dict(g=None), dict(o=None), dict(G=0), dict(G=-1), dict(n=0), dict(sdt=7),
               dict(sdt=-1), dict(g=(i32 * 3)(0, 0, 3)), dict(g=(i32 * 3)(0, 3, 2)), dict(g=(i32 * 3)(-1, 2, 3)), dict(mo=(i64 * 3)(0, -1, 32)),
               dict(t=d), dict(t=d, to=toff, tdt=2), dict(t=d, to=(i64 * 2)(48, -48)), dict(mean=d), dict(var=d.value + 47 * 4)):
        assert call(**kw) == RL_ERR_INVALID, kw
    assert b'overlaps' in L.lib.rl_last_error()
