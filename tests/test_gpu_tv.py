"""Total-variation regularised Richardson-Lucy on the MI355X (include/rlsted.h rl_deconv_set_tv): the device weights against the
numpy reference (tests/tv_reference.py) bit for bit, float64 plans against the reference loop -- plain and Biggs-Andrews --,
float32 plans against float64 on every loop a plan may choose, the state rules, the sweep's plan cache, the argument checks and
the gain at low dose.

Loop-level comparisons use lambda = 0.01, eps_rel = 0.1 on natural images only: the explicit TV step amplifies rounding
differences elsewhere, and correctness there is pinned at kernel level (test 1 here, tests/test_tv_cpu.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, max_rel
from oracle import line_sted_oracle as orc
from tv_reference import (AcceleratedRegularisedRL, RegularisedRL, device_means, low_dose_case, rmse, tv_seminorm, tv_weight)

pytestmark = pytest.mark.gpu

BA = 'biggs-andrews'
LAM, EPS = 0.01, 0.1


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


def _psfs(name):
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    return list(g[name])


def _objects():
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {k: o[k].astype(np.float64) for k in ('astronaut', 'rings', 'lines')}


def _stack(names):
    objs = _objects()
    return np.concatenate([objs[n] for n in names], axis=0)


def _noisy(psfs, obj, brightness, seed):
    """numpy Poisson draws of H(obj), per frame scaled to `brightness` (host, float64): list of (nz, ny, nx) per view."""
    obj = obj * (brightness / obj.sum(axis=(1, 2), keepdims=True))
    d = orc.Deconvolver(psfs)
    rng = np.random.default_rng(seed)
    return [rng.poisson(m) + 1e-9 for m in d.H(obj)]


def _plan(psfs, B, ny, nx, dtype='f64', tv=True, **kw):
    return _lib().DeconvPlan(psfs, B, ny, nx, dtype=dtype, tv_lambda=LAM if tv else None, tv_epsilon=EPS, **kw)


def _pixel_rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * np.max(np.abs(b)))))


def _device_weights(plan):
    """The plan's w buffer (rl_deconv_device_ptr which = 4) in its own element type."""
    L = _lib()
    arr = plan.device_array('tv_weight')
    n = plan.B * plan.ny * plan.nx
    out = np.empty(n, dtype=np.float64)
    L.check(L.lib.rl_device_download(plan.ctx.handle, ctypes.c_void_p(arr.__cuda_array_interface__['data'][0]), L.DTYPES[plan.dtype], n, L.ptr(out)))
    return out.reshape(plan.B, plan.ny, plan.nx).astype(np.float32 if plan.dtype == 'f32' else np.float64)


# ---------------------------------------------------------------------------------------------- 5. the device weights, bit for bit
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (33, 65), (64, 64), (107, 109)])
def test_device_weights_match_numpy_bit_for_bit(dtype, shape):
    """Three frames: odd sizes put frames and rows off 16-byte alignment.  w of the set estimate is what iterate(1) leaves in the
    plan's weight buffer.  Inputs: random, constant (w = 1 exactly), one with a 1e6 spike."""
    ny, nx = shape
    T = np.float32 if dtype == 'f32' else np.float64
    rng = np.random.default_rng(ny * 1000 + nx)
    psfs = _psfs('1p5x_lr/point_sted_psf')
    plan = _lib().DeconvPlan(psfs, 3, ny, nx, dtype=dtype)
    plan.set_measurement(rng.random((3, 1, ny, nx)) + 0.5)
    spike = rng.random((3, ny, nx))
    spike[:, rng.integers(ny), rng.integers(nx)] = 1e6
    for kind, x in (('random', rng.random((3, ny, nx)) * 3.0), ('constant', np.full((3, ny, nx), 2.75)), ('spike', spike)):
        for lam, eps in ((0.002, 0.1), (0.25, 1e-3), (0.01, 0.1)):
            plan.set_tv(lam, eps)
            plan.set_estimate(x)
            plan.iterate(1)
            xt = x.astype(T)
            want, den = tv_weight(xt, lam, eps, device_means(xt))
            got = _device_weights(plan)
            assert np.array_equal(got, want), (kind, lam, eps, float(np.max(np.abs(got - want))))
            assert np.all(den >= T(0.146))
            if kind == 'constant':
                assert np.all(got == 1)


# ---------------------------------------------------------------------------------------------- 6. f64 against the reference
@pytest.mark.parametrize('accel', [None, BA])
@pytest.mark.parametrize('brightness', [1e6, 1e9])
@pytest.mark.parametrize('views', [1, 3])
def test_f64_matches_numpy_reference(views, brightness, accel):
    psfs = _psfs('1p5x_lr/line_sted_psfs' if views == 3 else '1p5x_lr/point_sted_psf')
    obj = _stack(['astronaut', 'rings'])
    noisy = _noisy(psfs, obj, brightness, 7)
    ref = (AcceleratedRegularisedRL if accel else RegularisedRL)(psfs, noisy, LAM, EPS)
    plan = _plan(psfs, 2, 128, 128, acceleration=accel)
    plan.set_measurement(np.stack(noisy, axis=1))
    done = 0
    for K in (1, 2, 5, 20):
        plan.iterate(K - done)
        ref.iterate(K - done)
        done = K
        est = plan.estimate()
        print('f64 vs reference: views %d brightness %g accel %s K %d normwise %.3g pixelwise %.3g'
              % (views, brightness, accel, K, max_rel(est, ref.estimate), _pixel_rel(est, ref.estimate)))
        assert max_rel(est, ref.estimate) <= 1e-10, (K, max_rel(est, ref.estimate))
        assert _pixel_rel(est, ref.estimate) <= 1e-8, (K, _pixel_rel(est, ref.estimate))
    plain = _plan(psfs, 2, 128, 128, tv=False, acceleration=accel)
    plain.set_measurement(np.stack(noisy, axis=1))
    plain.iterate(20)
    assert max_rel(plain.estimate(), ref.estimate) > 1e-6      # (the regulariser did act)


# ---------------------------------------------------------------------------------------------- 7. f32 against f64, every loop
def _gauss(n, s):
    x = np.arange(n) - (n - 1) / 2
    return np.exp(-x ** 2 / (2 * s * s))


def _cases():
    sep = [np.outer(_gauss(7, 1.2), _gauss(5, 0.9))[None], np.outer(_gauss(5, 0.8), _gauss(7, 1.5))[None]]
    ring = np.outer(_gauss(7, 1.0), _gauss(7, 1.0)) + 0.3 * np.outer(_gauss(7, 2.5), _gauss(7, 0.6))
    return {
        'pair': (_psfs('1p5x_lr/point_sted_psf'), 512, 2, 20, {}, {'frame_pairs': True}),
        'per_frame': (_psfs('1p5x_lr/point_sted_psf'), 512, 2, 20, {'RLSTED_PAIR': '0'}, {'frame_pairs': False}),
        'views4': (_psfs('2p0x_lr/line_sted_psfs'), 512, 2, 20, {}, {'split_column_pass': False}),
        'split': (_psfs('2p0x_lr/line_sted_psfs'), 2048, 1, 5, {}, {'split_column_pass': True}),
        'separable': (sep, 512, 2, 20, {}, {'separable': True}),
        'direct': ([ring[None]], 512, 2, 20, {}, {'direct_stencil': True}),
    }


@pytest.mark.parametrize('case', ['pair', 'per_frame', 'views4', 'split', 'separable', 'direct'])
def test_f32_matches_f64_on_every_loop(case):
    """The f32 error with the regulariser on may be at most twice the error of the same plans with it off, measured here first,
    and never above the f32 contract 1e-5."""
    psfs, n, B, K, options, want = _cases()[case]
    base = _stack(['astronaut', 'rings'])[:B]
    obj = np.stack([np.kron(o, np.ones((n // 128, n // 128))) for o in base])
    p64 = _plan(psfs, B, n, n, 'f64', tv=False, options=options)
    p64.set_object(obj, [5e10 * (n / 128) ** 2] * B)
    p64.simulate(seed=11)
    meas = p64.measurement()
    p32 = _plan(psfs, B, n, n, 'f32', tv=False, options=options)
    err = {}
    for tv in (False, True):
        for p in (p32, p64):
            p.set_tv(LAM if tv else 0, EPS)
            p.set_measurement(meas)
            p.iterate(K)
        err[tv] = max_rel(p32.estimate(), p64.estimate())
    strat = p32.strategy()
    for k, v in want.items():
        assert strat[k] == v, (case, strat)
    print('f32 vs f64: %s TV off %.3g TV on %.3g' % (case, err[False], err[True]))
    assert err[False] <= 1e-5, (case, err)
    assert err[True] <= min(2 * err[False], 1e-5), (case, err)


# ---------------------------------------------------------------------------------------------- 8. behaviour and state
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_tv_off_again_is_plain_bit_for_bit(dtype):
    psfs = _psfs('1p5x_lr/point_sted_psf')
    obj = _stack(['astronaut', 'rings'])
    noisy = np.stack(_noisy(psfs, obj, 1e9, 9), axis=1)
    plain = _plan(psfs, 2, 128, 128, dtype, tv=False)
    plain.set_measurement(noisy)
    plain.iterate(6)
    want = plain.estimate()
    plan = _plan(psfs, 2, 128, 128, dtype)
    assert plan.tv() == (LAM, EPS)
    plan.set_measurement(noisy)
    plan.iterate(4)
    assert not np.array_equal(plan.estimate(), want)
    plan.set_tv(0, EPS)
    assert plan.tv()[0] == 0
    plan.set_measurement(noisy)
    plan.iterate(6)
    assert np.array_equal(plan.estimate(), want)
    # ... and switched off in the middle of a run: plain iterations continue from the regularised estimate
    plan.set_tv(LAM, EPS)
    plan.set_measurement(noisy)
    plan.iterate(3)
    x3 = plan.estimate()
    plan.set_tv(None)
    plan.iterate(3)
    plain.set_estimate(x3)
    plain.iterate(3)
    assert np.array_equal(plan.estimate(), plain.estimate())


@pytest.mark.parametrize('accel', [None, BA])
@pytest.mark.parametrize('views', [1, 3])
def test_split_runs_operators_between_until_and_batch_run(views, accel):
    psfs = _psfs('1p5x_lr/line_sted_psfs' if views == 3 else '1p5x_lr/point_sted_psf')
    obj = _stack(['astronaut', 'rings'])
    noisy = np.stack(_noisy(psfs, obj, 1e9, 5), axis=1)
    plan = _plan(psfs, 2, 128, 128, acceleration=accel)
    plan.set_measurement(noisy)
    plan.iterate(5)
    five = plan.estimate()
    plan.set_measurement(noisy)           # new data: from ones
    plan.iterate(3)
    plan.iterate(2)
    assert np.array_equal(plan.estimate(), five)
    plan.set_measurement(noisy)
    plan.iterate(3)
    plan.forward(obj)                     # H / H_t / the divergence in between change nothing
    plan.adjoint(noisy)
    plan.divergence()
    plan.iterate(2)
    assert np.array_equal(plan.estimate(), five)
    # iterate_until is the stepwise calls: a threshold nothing meets runs all 5 iterations and keeps the last check
    plan.set_measurement(noisy)
    info = plan.iterate_until(5, rule='discrepancy', threshold=-1.0, check_every=2)
    assert not info['stopped'].any() and np.all(info['iterations'] == 5)
    assert np.array_equal(plan.estimate(), five)
    plan.iterate(1)                       # ... and continues like a set estimate
    other = _plan(psfs, 2, 128, 128, acceleration=accel)
    other.set_measurement(noisy)
    other.set_estimate(five)
    other.iterate(1)
    assert np.array_equal(plan.estimate(), other.estimate())
    # rl_batch_run: simulate_keyed + iterate per task
    seeds, ids = [21, 22], [0, 1]
    out = plan.batch_run(list(obj), 1e9, seeds, ids, 5)
    other.set_object(obj, 1e9)
    other.simulate_keyed(seeds, ids)
    other.iterate(5)
    assert np.array_equal(out, other.estimate())


def test_batch_independence_f64():
    psfs = _psfs('1p5x_lr/line_sted_psfs')
    base = _stack(['astronaut', 'rings', 'lines'])
    frames = np.stack([np.rot90(base[i % 3], i // 3) for i in range(5)]) * np.linspace(0.5, 2.0, 5)[:, None, None]
    noisy = np.stack(_noisy(psfs, frames, 1e9, 4), axis=1)
    big, one = _plan(psfs, 5, 128, 128), _plan(psfs, 1, 128, 128)
    big.set_measurement(noisy)
    one.set_measurement(noisy[3:4])
    big.iterate(9)
    one.iterate(9)
    assert np.array_equal(big.estimate()[3], one.estimate()[0])


def test_set_estimate_and_new_data_follow_the_reference():
    psfs = _psfs('1p5x_lr/line_sted_psfs')
    obj = _stack(['astronaut', 'lines'])
    noisy, noisy2 = _noisy(psfs, obj, 1e9, 1), _noisy(psfs, obj, 1e9, 1001)
    ref = RegularisedRL(psfs, noisy, LAM, EPS)
    plan = _plan(psfs, 2, 128, 128)
    plan.set_measurement(np.stack(noisy, axis=1))
    plan.iterate(4)
    ref.iterate(4)
    x = ref.estimate * (1 + 0.2 * np.random.default_rng(1).random((2, 128, 128)))      # (a natural image still)
    plan.set_estimate(x)
    ref.set_estimate(x)
    plan.iterate(3)
    ref.iterate(3)
    assert max_rel(plan.estimate(), ref.estimate) <= 1e-10
    plan.set_measurement(np.stack(noisy2, axis=1))
    ref.set_measurement(noisy2)
    plan.iterate(6)
    ref.iterate(6)
    assert max_rel(plan.estimate(), ref.estimate) <= 1e-10
    assert _pixel_rel(plan.estimate(), ref.estimate) <= 1e-8


def test_sweep_plan_cache_keeps_tv_and_plain_apart():
    from rescan_line_sted_amd import sweep
    from rescan_line_sted_amd.line_sted_tools import Deconvolver
    objects = {k: v[0] for k, v in _objects().items() if k in ('astronaut', 'rings')}
    psf_sets = {'point': _psfs('1p5x_lr/point_sted_psf')}
    seeds, K = [3], 8
    tasks, plain1 = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64')
    tasks_t, tv = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64', tv_lambda=LAM, tv_epsilon=EPS)
    _, plain2 = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64')
    assert tasks == tasks_t
    assert np.array_equal(plain1, plain2)
    a = sweep.plan_for(psf_sets['point'], 2, (128, 128), 'f64')
    b = sweep.plan_for(psf_sets['point'], 2, (128, 128), 'f64', tv_lambda=LAM, tv_epsilon=EPS)
    c = sweep.plan_for(psf_sets['point'], 2, (128, 128), 'f64', tv_lambda=LAM, tv_epsilon=0.2)
    assert a is not b and b is not c and a.tv()[0] == 0 and b.tv() == (LAM, EPS) and c.tv() == (LAM, 0.2)
    assert sweep.plan_for(psf_sets['point'], 2, (128, 128), 'f64', tv_lambda=LAM, tv_epsilon=EPS) is b
    ids = sweep.object_ids(objects)
    for t, (o, p, s) in enumerate(tasks):
        d = Deconvolver(psf_sets[p], output_prefix=os.path.join(os.getcwd(), 'x'), dtype='f64', tv_lambda=LAM, tv_epsilon=EPS)
        keyed = _plan(psf_sets[p], 1, 128, 128, tv=False)
        keyed.set_object(objects[o][None], 1e9)
        keyed.simulate_keyed([s], [ids[o]])
        meas = keyed.measurement()
        d.noisy_measurement = [np.ascontiguousarray(meas[:, v]) for v in range(meas.shape[1])]
        d.iterate_many(K)
        assert max_rel(tv[t], d.estimate[0]) <= 1e-10, (tasks[t], max_rel(tv[t], d.estimate[0]))
        assert not np.array_equal(tv[t], plain1[t])


def test_invalid_arguments_are_rejected():
    L = _lib()
    psfs = _psfs('1p5x_lr/point_sted_psf')
    from rescan_line_sted_amd import sweep
    from rescan_line_sted_amd.line_sted_tools import Deconvolver, deconvolve
    for lam, eps in ((-0.01, 0.1), (0.26, 0.1), (float('nan'), 0.1), (0.01, 0.0), (0.01, -1.0), (0.01, float('inf')), (0.01, float('nan'))):
        with pytest.raises(ValueError):
            L.DeconvPlan(psfs, 1, 16, 16, tv_lambda=lam, tv_epsilon=eps)
        with pytest.raises(ValueError):
            Deconvolver(psfs, output_prefix=os.path.join(os.getcwd(), 'x'), tv_lambda=lam, tv_epsilon=eps)
        with pytest.raises(ValueError):
            deconvolve(np.ones((1, 1, 16, 16)), psfs, 1, tv_lambda=lam, tv_epsilon=eps)
        with pytest.raises(ValueError):
            sweep.plan_for(psfs, 1, (16, 16), tv_lambda=lam, tv_epsilon=eps)
    plan = L.DeconvPlan(psfs, 1, 16, 16, dtype='f64')
    for lam, eps in ((-0.01, 0.1), (0.26, 0.1), (float('nan'), 0.1), (0.01, 0.0), (0.01, float('inf')), (0.01, float('nan'))):
        assert L.lib.rl_deconv_set_tv(plan.handle, lam, eps) == -1         # RL_ERR_INVALID from the C ABI itself
    assert plan.tv() == (0.0, 0.1)                                          # the defaults, untouched
    with pytest.raises(L.RlstedError):
        plan.device_array('tv_weight')                                      # no weights before the mode was on
    plan.set_tv(0.25, 1e-3)
    assert plan.tv() == (0.25, 1e-3)


# ---------------------------------------------------------------------------------------------- 9. the gain
def test_low_dose_gain():
    """Astronaut at 6 photons per pixel, 200 iterations: the regularised estimate is closer to the truth (reference: 0.47 of the
    plain RMSE) and far less rough (0.36 of the plain TV seminorm)."""
    psfs, truth, noisy = low_dose_case(1e5)
    res = {}
    for tv in (False, True):
        plan = _plan(psfs, 1, 128, 128, tv=tv)
        plan.set_measurement(np.stack(noisy, axis=1))
        plan.iterate(200)
        res[tv] = plan.estimate()
    r = rmse(res[True], truth) / rmse(res[False], truth)
    t = tv_seminorm(res[True]) / tv_seminorm(res[False])
    print('low dose: RMSE ratio %.3f seminorm ratio %.3f' % (r, t))
    assert r <= 0.6, r
    assert t <= 0.5, t
