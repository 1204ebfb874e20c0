"""Biggs-Andrews accelerated Richardson-Lucy on the MI355X (include/rlsted.h rl_deconv_set_acceleration): float64 plans against
the numpy reference (tests/accel_reference.py), float32 plans against float64 on every loop a plan may choose, the history
rules, batch independence, the sweep and the gain in convergence."""
import os

import numpy as np
import pytest

from accel_reference import AcceleratedRL, i_divergence
from conftest import GOLDEN, fuzz_seeds, max_rel
from oracle import line_sted_oracle as orc

pytestmark = pytest.mark.gpu

BA = 'biggs-andrews'


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


def _psfs(name):
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    return list(g[name])


def _objects():
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {k: o[k].astype(np.float64) for k in ('astronaut', 'rings', 'lines')} | {'cat': o['cat'].astype(np.float64)[:, 16:144, 16:144]}


def _stack(names):
    objs = _objects()
    return np.concatenate([objs[n] for n in names], axis=0)


def _noisy(psfs, obj, brightness, seed):
    """numpy Poisson draws of H(obj), per frame scaled to `brightness` (host, float64): list of (nz, ny, nx) per view."""
    obj = obj * (brightness / obj.sum(axis=(1, 2), keepdims=True))
    d = orc.Deconvolver(psfs)
    rng = np.random.default_rng(seed)
    return [rng.poisson(m) + 1e-9 for m in d.H(obj)]


def _plan(psfs, B, ny, nx, dtype='f64', acceleration=BA, options=None):
    return _lib().DeconvPlan(psfs, B, ny, nx, dtype=dtype, acceleration=acceleration, options=options)


def _pixel_rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * np.max(np.abs(b)))))


# ---------------------------------------------------------------------------------------------- 1. f64 against the reference
@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('seed', fuzz_seeds(1))
def test_random_f64_matches_numpy_reference(views, seed):
    psfs = _psfs('1p5x_lr/line_sted_psfs' if views == 3 else '1p5x_lr/point_sted_psf')
    rng = np.random.default_rng(seed)
    names = ['astronaut', 'rings', 'lines', 'cat']
    obj = _stack([names[i] for i in rng.permutation(4)[:2]])
    noisy = _noisy(psfs, obj, float(10 ** rng.uniform(6, 10)), seed)
    ref = AcceleratedRL(psfs, noisy)
    plan = _plan(psfs, obj.shape[0], 128, 128)
    plan.set_measurement(np.stack(noisy, axis=1))
    done = 0
    for K in (1, 2, 3, 5, 20):
        plan.iterate(K - done)
        ref.iterate(K - done)
        done = K
        est = plan.estimate()
        assert max_rel(est, ref.estimate) <= 1e-10, (K, max_rel(est, ref.estimate))
        assert _pixel_rel(est, ref.estimate) <= 1e-8, (K, _pixel_rel(est, ref.estimate))
        assert np.max(np.abs(plan.alpha() - ref.alpha)) <= 1e-9, (K, plan.alpha(), ref.alpha)
    assert np.all(ref.alpha > 0)     # (the extrapolation did act)


# ---------------------------------------------------------------------------------------------- 2. f32 against f64, every loop
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
    psfs, n, B, K, options, want = _cases()[case]
    base = _stack(['astronaut', 'rings'])[:B]
    obj = np.stack([np.kron(o, np.ones((n // 128, n // 128))) for o in base])
    p64 = _plan(psfs, B, n, n, 'f64', options=options)
    p64.set_object(obj, [5e10 * (n / 128) ** 2] * B)
    p64.simulate(seed=11)
    meas = p64.measurement()
    p32 = _plan(psfs, B, n, n, 'f32', options=options)
    p32.set_measurement(meas)
    p32.iterate(K)
    p64.iterate(K)
    strat = p32.strategy()
    for k, v in want.items():
        assert strat[k] == v, (case, strat)
    err = max_rel(p32.estimate(), p64.estimate())
    assert err <= 1e-5, (case, err)
    assert np.all(p64.alpha() > 0) or K < 3


# ---------------------------------------------------------------------------------------------- 3. the history rules
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('views', [1, 3])
def test_split_runs_and_operators_between(dtype, views):
    psfs = _psfs('1p5x_lr/line_sted_psfs' if views == 3 else '1p5x_lr/point_sted_psf')
    obj = _stack(['astronaut', 'rings'])
    noisy = np.stack(_noisy(psfs, obj, 1e9, 5), axis=1)
    plan = _plan(psfs, 2, 128, 128, dtype)
    plan.set_measurement(noisy)
    plan.iterate(5)
    five, a5 = plan.estimate(), plan.alpha()
    plan.set_measurement(noisy)           # new data: from ones, no history
    plan.iterate(3)
    plan.iterate(2)
    assert np.array_equal(plan.estimate(), five)
    assert np.array_equal(plan.alpha(), a5)
    plan.set_measurement(noisy)
    plan.iterate(3)
    plan.forward(obj)                     # H / H_t in between leave the history alone
    plan.adjoint(noisy)
    plan.iterate(2)
    assert np.array_equal(plan.estimate(), five)


@pytest.mark.parametrize('seed', fuzz_seeds(1))
def test_random_set_estimate_and_new_data_reset_history(seed):
    psfs = _psfs('1p5x_lr/line_sted_psfs')
    obj = _stack(['astronaut', 'lines'])
    noisy = _noisy(psfs, obj, 1e9, seed)
    noisy2 = _noisy(psfs, obj, 1e9, seed + 1000)
    ref = AcceleratedRL(psfs, noisy)
    plan = _plan(psfs, 2, 128, 128)
    plan.set_measurement(np.stack(noisy, axis=1))
    plan.iterate(4)
    ref.iterate(4)
    x = np.random.default_rng(seed).random((2, 128, 128)) * np.max(ref.estimate)
    plan.set_estimate(x)
    ref.set_estimate(x)
    plan.iterate(1)
    ref.iterate(1)
    assert np.all(plan.alpha() == 0)
    plan.iterate(3)
    ref.iterate(3)
    assert max_rel(plan.estimate(), ref.estimate) <= 1e-10
    plan.set_measurement(np.stack(noisy2, axis=1))
    ref.set_measurement(noisy2)
    plan.iterate(6)
    ref.iterate(6)
    assert max_rel(plan.estimate(), ref.estimate) <= 1e-10
    assert np.max(np.abs(plan.alpha() - ref.alpha)) <= 1e-9


def test_deconvolver_iterate_equals_iterate_many():
    from rescan_line_sted_amd.line_sted_tools import Deconvolver
    psfs = [p for p in _psfs('1p5x_lr/line_sted_psfs')]
    obj = _stack(['rings'])
    runs = []
    for many in (False, True):
        d = Deconvolver(psfs, output_prefix=os.path.join(os.getcwd(), 'x'), dtype='f64', acceleration=BA)
        d.create_data_from_object(obj.copy(), total_brightness=1e9, random_seed=2)
        if many:
            d.iterate_many(7)
        else:
            for i in range(7):
                d.iterate()
                if i == 3:
                    d.H(d.estimate)       # the operators (and a look at the estimate) in between change nothing
                    d.H_t(d.noisy_measurement)
        runs.append(d.estimate.copy())
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_acceleration_off_again_is_plain_bit_for_bit(dtype):
    psfs = _psfs('1p5x_lr/point_sted_psf')
    obj = _stack(['astronaut', 'rings'])
    noisy = np.stack(_noisy(psfs, obj, 1e9, 9), axis=1)
    plain = _plan(psfs, 2, 128, 128, dtype, acceleration=None)
    plain.set_measurement(noisy)
    plain.iterate(6)
    want = plain.estimate()
    plan = _plan(psfs, 2, 128, 128, dtype)
    plan.set_measurement(noisy)
    plan.iterate(4)
    assert not np.array_equal(plan.estimate(), want)
    plan.set_acceleration(None)
    plan.set_measurement(noisy)
    plan.iterate(6)
    assert np.array_equal(plan.estimate(), want)
    # ... and switched off in the middle of a run: plain iterations continue from the accelerated estimate
    plan.set_acceleration(BA)
    plan.set_measurement(noisy)
    plan.iterate(3)
    x3 = plan.estimate()
    plan.set_acceleration(None)
    plan.iterate(3)
    plain.set_estimate(x3)
    plain.iterate(3)
    assert np.array_equal(plan.estimate(), plain.estimate())


# ---------------------------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize('seed', fuzz_seeds(1))
def test_random_batch_independence_f64(seed):
    psfs = _psfs('1p5x_lr/line_sted_psfs')
    rng = np.random.default_rng(seed)
    base = _stack(['astronaut', 'rings', 'lines', 'cat'])
    frames = np.stack([np.rot90(base[i % 4], i // 4 + 1) if i >= 4 else base[i] for i in range(7)])
    frames = frames * rng.uniform(0.5, 2.0, size=(7, 1, 1))
    noisy = np.stack(_noisy(psfs, frames, 1e9, seed), axis=1)
    pick = int(rng.integers(7))
    big, one = _plan(psfs, 7, 128, 128), _plan(psfs, 1, 128, 128)
    big.set_measurement(noisy)
    one.set_measurement(noisy[pick:pick + 1])
    big.iterate(9)
    one.iterate(9)
    assert np.array_equal(big.estimate()[pick], one.estimate()[0])
    assert np.array_equal(big.alpha()[pick], one.alpha()[0])
    ids = list(range(7))
    seeds = [int(s) for s in rng.integers(0, 2 ** 31, size=7)]
    out_big = big.batch_run(list(frames), 1e9, seeds, ids, 9)
    out_one = one.batch_run([frames[pick]], 1e9, [seeds[pick]], [ids[pick]], 9)
    assert np.array_equal(out_big[pick], out_one[0])
    plain = _plan(psfs, 7, 128, 128, acceleration=None)
    assert not np.array_equal(plain.batch_run(list(frames), 1e9, seeds, ids, 9)[pick], out_big[pick])


# ---------------------------------------------------------------------------------------------- 5. the sweep
def test_sweep_accelerated_and_plan_cache_key():
    from rescan_line_sted_amd import sweep
    from rescan_line_sted_amd.line_sted_tools import Deconvolver
    objects = {k: v[0] for k, v in _objects().items() if k in ('astronaut', 'rings')}
    psf_sets = {'point': _psfs('1p5x_lr/point_sted_psf'), 'line': _psfs('1p5x_lr/line_sted_psfs')}
    seeds, K = [3, 4], 12
    tasks, plain1 = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64')
    tasks_a, acc = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64', acceleration=BA)
    _, plain2 = sweep.figure_2_sweep(objects, psf_sets, seeds, K, total_brightness=1e9, dtype='f64')
    assert tasks == tasks_a
    assert np.array_equal(plain1, plain2)
    ids = sweep.object_ids(objects)
    for t, (o, p, s) in enumerate(tasks):
        keyed = _lib().DeconvPlan(psf_sets[p], 1, 128, 128, dtype='f64')
        keyed.set_object(objects[o][None], 1e9)
        keyed.simulate_keyed([s], [ids[o]])
        meas = keyed.measurement()
        d = Deconvolver(psf_sets[p], output_prefix=os.path.join(os.getcwd(), 'x'), dtype='f64', acceleration=BA)
        d.noisy_measurement = [np.ascontiguousarray(meas[:, v]) for v in range(meas.shape[1])]
        d.iterate_many(K)
        assert max_rel(acc[t], d.estimate[0]) <= 1e-10, (tasks[t], max_rel(acc[t], d.estimate[0]))
        assert not np.array_equal(acc[t], plain1[t])


# ---------------------------------------------------------------------------------------------- 6. convergence
@pytest.mark.parametrize('psf_set', ['1p5x_lr/line_sted_psfs', '1p5x_lr/point_sted_psf'])
def test_accelerated_k32_fits_better_than_plain_k64(psf_set):
    psfs = _psfs(psf_set)
    obj = _objects()['astronaut']
    d = orc.Deconvolver(psfs)
    div = {}
    for mode, K in ((None, 64), (BA, 32)):
        plan = _plan(psfs, 1, 128, 128, 'f32', acceleration=mode)
        plan.set_object(obj, 5e10)
        plan.simulate(seed=1)
        plan.iterate(K)
        meas = plan.measurement()
        div[mode] = i_divergence([meas[:, v] for v in range(meas.shape[1])], d.H(plan.estimate()))
    assert div[BA] < div[None], div
