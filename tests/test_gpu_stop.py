"""The Poisson I-divergence on the MI355X and Richardson-Lucy with a stopping rule per frame (include/rlsted.h rl_deconv_divergence,
rl_deconv_iterate_until): D against numpy on the plan's own data on every strategy, a float64 plan's D and stop iterations against
the oracle (tests/stop_reference.py), iterate_until against the sequence of public calls that defines it, batch independence, the
state rules, and the default path left as it was."""
import os

import numpy as np
import pytest

import stop_reference as sr
from conftest import GOLDEN, fuzz_seeds, max_rel

pytestmark = pytest.mark.gpu

BA = 'biggs-andrews'
RL_ERR_INVALID, RL_ERR_STATE = -1, -4
STATE_BYTES = 24          # StopFrame of csrc/stop_kernels.hpp: two doubles, two ints


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


def _plan(psfs, B, ny, nx, dtype='f64', acceleration=None, options=None):
    return _lib().DeconvPlan(psfs, B, ny, nx, dtype=dtype, acceleration=acceleration, options=options)


def _objects():
    o = np.load(os.path.join(GOLDEN, 'objects.npz'))
    return {k: o[k].astype(np.float64) for k in ('astronaut', 'rings', 'lines')} | {'cat': o['cat'].astype(np.float64)[:, 16:144, 16:144]}


def _stack(names):
    objs = _objects()
    return np.concatenate([objs[n] for n in names], axis=0)


def _wrapped(obj, n):
    """(B, 128, 128) objects continued periodically to n x n (n = 200: transform length 256, the shortest that has the pair loop)."""
    pad = (n - obj.shape[1]) // 2
    return np.pad(obj, ((0, 0), (pad, pad), (pad, pad)), mode='wrap')


def _gauss(n, s):
    x = np.arange(n) - (n - 1) / 2
    return np.exp(-x ** 2 / (2 * s * s))


def _itemsize(dtype):
    return 4 if dtype == 'f32' else 8


def _check_divergence(plan, dtype, tag):
    """plan.divergence() against numpy on the plan's own stored measurement and its own forward(estimate())."""
    est = plan.estimate()
    D = plan.divergence()
    assert np.array_equal(plan.estimate(), est)              # the estimate stays
    meas, pred = plan.measurement(), plan.forward(est)
    N = meas[0].size
    L = sr.chain_length(N, _itemsize(dtype))                 # vectors per thread * W + log2(threads) + workgroups per frame
    for f in range(plan.B):
        want, bound = sr.divergence(meas[f], pred[f]), sr.summation_bound(meas[f], pred[f], L)
        print('%s frame %d: D %.17g numpy %.17g diff %.3g bound %.3g (L = %d)' % (tag, f, D[f], want, abs(D[f] - want), bound, L))
        assert abs(D[f] - want) <= bound, (tag, f, D[f], want, bound)
    return D


# ---------------------------------------------------------------------------------------------- 4. D against numpy, every strategy
def _strategy_cases():
    sep = [np.outer(_gauss(7, 1.2), _gauss(5, 0.9))[None], np.outer(_gauss(5, 0.8), _gauss(7, 1.5))[None]]
    ring = np.outer(_gauss(7, 1.0), _gauss(7, 1.0)) + 0.3 * np.outer(_gauss(7, 2.5), _gauss(7, 0.6))
    return {   # PSFs, size, batches to draw from, iterations at most, options, what an f32 plan's strategy must report
        'pair': (sr.psf_set(sr.POINT), 512, (2, 4), 6, {}, {'frame_pairs': True}),
        'per_frame': (sr.psf_set(sr.POINT), 512, (1, 2, 3), 6, {'RLSTED_PAIR': '0'}, {'frame_pairs': False}),
        'views4': (sr.psf_set(sr.LINE), 512, (1, 2, 3), 6, {}, {'split_column_pass': False}),
        'split': (sr.psf_set(sr.LINE), 2048, (1,), 2, {}, {'split_column_pass': True}),
        'separable': (sep, 512, (1, 2, 3), 6, {}, {'separable': True}),
        'direct': ([ring[None]], 512, (1, 2, 3), 6, {}, {'direct_stencil': True}),
    }


@pytest.mark.parametrize('acceleration', [None, BA])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('case', ['pair', 'per_frame', 'views4', 'split', 'separable', 'direct'])
@pytest.mark.parametrize('seed', fuzz_seeds(1))
def test_random_divergence_matches_numpy_on_every_strategy(seed, case, dtype, acceleration):
    psfs, n, batches, kmax, options, want = _strategy_cases()[case]
    rng = np.random.default_rng([seed, len(case), _itemsize(dtype)])
    B = int(rng.choice(batches))
    names = ['astronaut', 'rings', 'lines', 'cat']
    base = _stack([names[i] for i in rng.integers(0, 4, size=B)])
    obj = np.stack([np.kron(o, np.ones((n // 128, n // 128))) for o in base])
    dose = 10 ** rng.uniform(6, 10) * (n / 128) ** 2
    doses = dose * rng.uniform(1.0, 3.0, size=B)             # (partners of comparable level: the pair loop runs)
    plan = _plan(psfs, B, n, n, dtype, acceleration, options)
    plan.set_object(obj, doses)
    plan.simulate(seed=seed + 1)
    if dtype == 'f32':
        strat = plan.strategy()
        for k, v in want.items():
            assert strat[k] == v, (case, strat)
    plan.iterate(int(rng.integers(1, kmax + 1)))
    _check_divergence(plan, dtype, '%s %s %s' % (case, dtype, acceleration))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('views', [1, 4])
@pytest.mark.parametrize('seed', fuzz_seeds(2))
def test_random_divergence_shapes_batches_doses(seed, views, dtype):
    """Any shape: odd frame sizes put every second frame off 16-byte alignment and leave a partial last vector; low doses bring
    zeros into the measurement (1e-9 after the draw) and predictions near zero."""
    rng = np.random.default_rng([seed, views, _itemsize(dtype)])
    ny, nx, B = int(rng.integers(33, 200)), int(rng.integers(33, 200)), int(rng.integers(1, 6))
    psfs = sr.psf_set(sr.LINE if views == 4 else sr.POINT)
    obj = rng.random((B, ny, nx)) ** 4
    plan = _plan(psfs, B, ny, nx, dtype, BA if seed % 2 else None)
    plan.set_object(obj, 10 ** rng.uniform(2.5, 9, size=B))
    plan.simulate(seed=seed)
    plan.iterate(int(rng.integers(1, 8)))
    _check_divergence(plan, dtype, 'shape %dx%d B %d V %d %s' % (ny, nx, B, views, dtype))


# ---------------------------------------------------------------------------------------------- 5. f64 D against the oracle
@pytest.mark.parametrize('case', list(sr.TABLE), ids=lambda c: '%s-%s-%g' % (c[0], c[1].split('/')[1][:5], c[2]))
def test_f64_divergence_matches_oracle(case):
    """D after K = 1, 5, 20 iterations against the oracle on the same measurement.  Bound, per case and K, from the float64 contract
    (the plan's prediction within 1e-10 of the oracle's maximum, normwise) through dD/dp = 1 - m / p:
    |D - D_oracle| <= sum|1 - m / p| * 1e-10 * max p, all from oracle quantities (stop_reference.contract_bound)."""
    psfs, meas = sr.case_measurement(*case)
    trace = {k: (d, pred) for k, d, _, pred in sr.oracle_trace(psfs, meas, 20, 1, keep_estimates=False)}
    plan = _plan(psfs, 1, 128, 128, 'f64')
    plan.set_measurement(np.stack(meas, axis=1))
    done = 0
    for K in (1, 5, 20):
        plan.iterate(K - done)
        done = K
        D = plan.divergence()[0]
        want, pred = trace[K]
        bound = sr.contract_bound(meas, pred)
        print('%s K %d: D %.17g oracle %.17g |diff| / D %.3g bound / D %.3g' % (case, K, D, want, abs(D - want) / want, bound / want))
        assert abs(D - want) <= bound, (case, K, D, want, bound)


# ---------------------------------------------------------------------------------------------- 6. iterate_until == the public calls
def _stepwise(plan, k_max, rule, threshold, check_every):
    """The sequence rl_deconv_iterate_until is defined as, by public calls; the rule in numpy on the returned doubles."""
    B, N = plan.B, plan.V * plan.ny * plan.nx
    its, div, stopped = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B, dtype=bool)
    est = np.zeros((B, plan.ny, plan.nx))
    prev, done = None, 0
    while done < k_max and not stopped.all():
        c = min(check_every, k_max - done)
        plan.iterate(c)
        done += c
        D, x = plan.divergence(), plan.estimate()
        for f in range(B):
            if stopped[f]:
                continue
            est[f], its[f], div[f] = x[f], done, D[f]
            stopped[f] = sr.rule_met(rule, threshold, N, D[f], None if prev is None else prev[f])
        prev = D
    return est, {'iterations': its, 'divergence': div, 'stopped': stopped}


def _assert_same_run(got_est, got, want_est, want, tag):
    assert np.array_equal(got['iterations'], want['iterations']), (tag, got, want)
    assert np.array_equal(got['stopped'], want['stopped']), (tag, got, want)
    assert np.array_equal(got['divergence'], want['divergence'], equal_nan=True), (tag, got, want)
    assert np.array_equal(got_est, want_est), tag


@pytest.mark.parametrize('rule', [sr.DISCREPANCY, sr.RELATIVE])
@pytest.mark.parametrize('check_every', [1, 3, 7])
@pytest.mark.parametrize('acceleration', [None, BA])
@pytest.mark.parametrize('views', [1, 4])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_iterate_until_is_the_stepwise_sequence_bit_for_bit(dtype, views, acceleration, check_every, rule):
    psfs = sr.psf_set(sr.LINE if views == 4 else sr.POINT)
    obj = _stack(['lines', 'astronaut', 'rings', 'lines'] if views == 1 else ['lines', 'astronaut', 'rings'])
    n = 200 if views == 1 else 128                                # (single view: a size whose f32 plan pairs its frames)
    obj = _wrapped(obj, n)
    doses = [d * (n / 128) ** 2 for d in [1e5, 2e5, 2e6, 1e6][:obj.shape[0]]]
    B, k_max = obj.shape[0], 20                                  # (20 is no multiple of 3 or 7: the last run of iterations is shorter)
    threshold = 1.0 if rule == sr.DISCREPANCY else 2e-3
    runs = []
    for until in (True, False):
        plan = _plan(psfs, B, n, n, dtype, acceleration)
        plan.set_object(obj, doses)
        plan.simulate(seed=4)
        if until:
            assert plan.strategy()['frame_pairs'] == (dtype == 'f32' and views == 1)
            info = plan.iterate_until(k_max, rule=rule, threshold=threshold, check_every=check_every)
            runs.append((plan.estimate(), info))
        else:
            runs.append(_stepwise(plan, k_max, rule, threshold, check_every))
    tag = (dtype, views, acceleration, check_every, rule, runs[0][1])
    _assert_same_run(runs[0][0], runs[0][1], runs[1][0], runs[1][1], tag)
    assert runs[0][1]['iterations'].max() <= k_max and runs[0][1]['iterations'].min() >= min(check_every, k_max)


# ---------------------------------------------------------------------------------------------- 7. the study's batches
LINE_ROWS = [('lines', sr.LINE, 1e6), ('astronaut', sr.LINE, 1e6), ('lines', sr.LINE, 1e7), ('astronaut', sr.LINE, 1e8)]
POINT_ROWS = [('lines', sr.POINT, 1e5), ('astronaut', sr.POINT, 1e5), ('lines', sr.POINT, 1e6), ('astronaut', sr.POINT, 1e8)]
EXPECTED = {   # (iterations reported, stopped) per frame: discrepancy rule at t = 1, relative rule at t = 1e-3; check_every 2, k_max 60
    'line': {sr.DISCREPANCY: ([14, 22, 60, 60], [1, 1, 0, 0]), sr.RELATIVE: ([18, 26, 44, 60], [1, 1, 1, 0])},
    'point': {sr.DISCREPANCY: ([8, 34, 60, 60], [1, 1, 0, 0]), sr.RELATIVE: ([12, 26, 28, 60], [1, 1, 1, 0])},
}
THRESHOLD = {sr.DISCREPANCY: 1.0, sr.RELATIVE: 1e-3}


def _oracle_batch(rows):
    traces = [sr.case_trace(*row) for row in rows]
    meas = np.concatenate([np.stack(t[1], axis=1) for t in traces], axis=0)      # (4, V, 128, 128)
    return traces[0][0], meas, [t[1] for t in traces], [t[2] for t in traces]


def _oracle_decisions(meas_f, trace, rule):
    """The oracle's stop of one frame, after asserting that no decision is closer to its threshold than 100 x the bound on
    |D_device - D_oracle| (test_f64_divergence_matches_oracle's; for the relative decrease the sum of two, relative to D_prev)."""
    N = sum(m.size for m in meas_f)
    D = [t[1] for t in trace]
    b = [sr.contract_bound(meas_f, t[3]) for t in trace]
    for i in range(len(D)):
        if rule == sr.DISCREPANCY:
            dist, bound = abs(2.0 * D[i] / N - 1.0), 2.0 * b[i] / N
        elif i == 0:
            continue
        else:
            dist, bound = abs((D[i - 1] - D[i]) / D[i - 1] - 1e-3), (b[i] + b[i - 1]) / D[i - 1]
        assert dist >= 100.0 * bound, (rule, trace[i][0], dist, bound)
    i = sr.first_stop(D, rule, THRESHOLD[rule], N)
    return (trace[-1], 0) if i is None else (trace[i], 1)


@pytest.mark.parametrize('rule', [sr.DISCREPANCY, sr.RELATIVE])
@pytest.mark.parametrize('batch', ['line', 'point'])
def test_f64_stops_where_the_oracle_stops(batch, rule):
    psfs, meas, meas_f, traces = _oracle_batch(LINE_ROWS if batch == 'line' else POINT_ROWS)
    want = [_oracle_decisions(meas_f[f], traces[f], rule) for f in range(4)]      # (asserts the margins on the oracle first)
    assert ([w[0][0] for w in want], [w[1] for w in want]) == EXPECTED[batch][rule]
    plan = _plan(psfs, 4, 128, 128, 'f64')
    plan.set_measurement(meas)
    info = plan.iterate_until(60, rule=rule, threshold=THRESHOLD[rule], check_every=2)
    est = plan.estimate()
    print(batch, rule, info)
    assert list(info['iterations']) == EXPECTED[batch][rule][0]
    assert [int(s) for s in info['stopped']] == EXPECTED[batch][rule][1]
    for f in range(4):
        (k, D, x, pred), _ = want[f]
        assert max_rel(est[f], x[0]) <= 1e-10, (batch, rule, f, max_rel(est[f], x[0]))
        assert abs(info['divergence'][f] - D) <= sr.contract_bound(meas_f[f], pred), (batch, rule, f, info['divergence'][f], D)


@pytest.mark.parametrize('rule', [sr.DISCREPANCY, sr.RELATIVE])
def test_f32_point_batch_is_the_stepwise_sequence(rule):
    """The f32 plan of the study's single-view batch, against the sequence of public calls (not against the oracle).  At 128 x 128 the
    transform length is 192, which has no pair loop: the plan runs its per-frame loop (the pair loop against the same sequence:
    test_iterate_until_is_the_stepwise_sequence_bit_for_bit, at 200 x 200)."""
    psfs, meas, _, _ = _oracle_batch(POINT_ROWS)
    runs = []
    for until in (True, False):
        plan = _plan(psfs, 4, 128, 128, 'f32')
        plan.set_measurement(meas)
        if until:
            info = plan.iterate_until(60, rule=rule, threshold=THRESHOLD[rule], check_every=2)
            runs.append((plan.estimate(), info))
        else:
            runs.append(_stepwise(plan, 60, rule, THRESHOLD[rule], 2))
    print(rule, runs[0][1])
    _assert_same_run(runs[0][0], runs[0][1], runs[1][0], runs[1][1], rule)


# ---------------------------------------------------------------------------------------------- 8. batch independence
@pytest.mark.parametrize('rule', [sr.DISCREPANCY, sr.RELATIVE])
@pytest.mark.parametrize('seed', fuzz_seeds(1))
def test_random_batch_independence_f64(seed, rule):
    psfs = sr.psf_set('1p5x_lr/line_sted_psfs')
    rng = np.random.default_rng(seed)
    base = _stack(['astronaut', 'rings', 'lines', 'cat'])
    frames = np.stack([np.rot90(base[i % 4], i // 4 + 1) if i >= 4 else base[i] for i in range(7)])
    big, one = _plan(psfs, 7, 128, 128), _plan(psfs, 1, 128, 128)
    big.set_object(frames, 10 ** rng.uniform(4, 6, size=7))
    big.simulate(seed=seed)
    noisy = big.measurement()
    order = rng.permutation(7)
    pick = int(rng.integers(7))
    big.set_measurement(noisy[order])
    one.set_measurement(noisy[order][pick:pick + 1])
    big.iterate(4)
    one.iterate(4)
    assert big.divergence()[pick] == one.divergence()[0]
    threshold = 1.0 if rule == sr.DISCREPANCY else 3e-3
    a = big.iterate_until(40, rule=rule, threshold=threshold, check_every=2)
    b = one.iterate_until(40, rule=rule, threshold=threshold, check_every=2)
    print(a, b)
    assert a['iterations'][pick] == b['iterations'][0] and a['stopped'][pick] == b['stopped'][0]
    assert a['divergence'][pick] == b['divergence'][0]
    assert np.array_equal(big.estimate()[pick], one.estimate()[0])
    assert a['stopped'].any()                               # (the rule did act)


# ---------------------------------------------------------------------------------------------- 9. state
def _error_code(fn, *args, **kw):
    with pytest.raises(_lib().RlstedError) as e:
        fn(*args, **kw)
    return int(str(e.value).split('error ')[1].split(':')[0])


@pytest.mark.parametrize('dtype,views,acceleration', [('f32', 1, None), ('f32', 4, BA), ('f64', 1, BA), ('f64', 4, None)])
def test_state_rules(dtype, views, acceleration):
    psfs = sr.psf_set(sr.LINE if views == 4 else sr.POINT)
    obj = _stack(['astronaut', 'lines'])
    plan = _plan(psfs, 2, 128, 128, dtype, acceleration)
    assert _error_code(plan.divergence) == RL_ERR_STATE                          # no measurement
    assert _error_code(plan.iterate_until, 5) == RL_ERR_STATE
    plan.set_object(obj, [1e6, 2e6])
    plan.simulate(seed=2)
    assert _error_code(plan.divergence) == RL_ERR_STATE                          # no estimate
    for bad in ((0, 1, 1, 1.0), (5, 0, 1, 1.0), (5, 1, 0, 1.0), (5, 1, 3, 1.0), (5, 1, 1, float('nan'))):
        assert _lib().lib.rl_deconv_iterate_until(plan.handle, bad[0], bad[1], bad[2], bad[3], None, None, None) == RL_ERR_INVALID
    with pytest.raises(ValueError):
        plan.iterate_until(5, rule='chi2')
    # device_bytes grows by exactly the new buffers, on first use
    es, n, B = _itemsize(dtype), 128 * 128, 2
    bytes0 = plan.info()['device_bytes']
    plan.iterate(3)
    assert plan.info()['device_bytes'] == bytes0
    plan.divergence()
    bytes1 = plan.info()['device_bytes']
    assert bytes1 - bytes0 == B * sr.stop_blocks(views * n, es) * 8 + B * 8        # the partials, the frames' D
    plan.divergence()
    assert plan.info()['device_bytes'] == bytes1
    # divergence between iterations is forward between iterations
    meas = plan.measurement()
    plan.iterate(2)
    want = plan.estimate()
    plan.set_measurement(meas)
    plan.iterate(3)
    plan.forward(obj)
    plan.iterate(2)
    assert np.array_equal(plan.estimate(), want)
    # iterate_until, then iterate: continues as from a set estimate
    plan.set_measurement(meas)
    info = plan.iterate_until(9, rule=sr.RELATIVE, threshold=5e-2, check_every=2)
    bytes2 = plan.info()['device_bytes']
    assert bytes2 - bytes1 == B * n * es + 2 * B * STATE_BYTES                    # the kept estimates, the double-buffered state
    result = plan.estimate()
    assert plan.last_ms()['iterate_ms'] > 0
    plan.iterate(3)
    got = plan.estimate()
    plan.set_estimate(result)
    plan.iterate(3)
    assert np.array_equal(plan.estimate(), got)
    plan.set_measurement(meas)
    plan.iterate_until(9, rule=sr.RELATIVE, threshold=5e-2, check_every=2)
    assert plan.info()['device_bytes'] == bytes2
    assert np.array_equal(plan.estimate(), result)
    # the device view of the estimate shows the kept estimates too
    out = np.zeros(B * n)
    lib = _lib()
    p, cnt, dt = lib._vp(), lib._c.c_size_t(), lib._i()
    lib.check(lib.lib.rl_deconv_device_ptr(plan.handle, 0, lib._c.byref(p), lib._c.byref(cnt), lib._c.byref(dt)))
    lib.check(lib.lib.rl_device_download(plan.ctx.handle, p, dt.value, B * n, lib.ptr(out)))
    assert np.array_equal(out.reshape(result.shape), result)
    # from an estimate that exists: continues from it (iterations count from the start of the call)
    plan.set_estimate(result)
    info2 = plan.iterate_until(4, rule=sr.DISCREPANCY, threshold=-1.0, check_every=3)
    assert list(info2['iterations']) == [4, 4] and not info2['stopped'].any()
    assert info['iterations'].max() <= 9


def test_deconvolve_until_returns_what_the_plan_returns():
    from rescan_line_sted_amd.line_sted_tools import deconvolve_until
    psfs, meas, _, _ = _oracle_batch(POINT_ROWS)
    for kw in ({}, {'acceleration': BA}):
        plan = _plan(psfs, 4, 128, 128, 'f32')
        est, info = deconvolve_until(meas, psfs, 30, rule=sr.RELATIVE, threshold=1e-3, check_every=2, plan=plan, **kw)
        other = _plan(psfs, 4, 128, 128, 'f32', kw.get('acceleration'))
        other.set_measurement(meas)
        want = other.iterate_until(30, rule=sr.RELATIVE, threshold=1e-3, check_every=2)
        assert np.array_equal(est, other.estimate())
        for k in ('iterations', 'divergence', 'stopped'):
            assert np.array_equal(info[k], want[k])
    est2, info2 = deconvolve_until(meas, psfs, 30, rule=sr.RELATIVE, threshold=1e-3, check_every=2, dtype='f32', acceleration=BA)
    assert np.array_equal(est2, est) and np.array_equal(info2['iterations'], info['iterations'])


# ---------------------------------------------------------------------------------------------- 10. the default path
@pytest.mark.parametrize('dtype,views', [('f32', 1), ('f32', 4), ('f64', 1)])
def test_default_path_untouched_by_the_new_calls(dtype, views):
    psfs = sr.psf_set(sr.LINE if views == 4 else sr.POINT)
    n = 200 if views == 1 else 128
    obj = _wrapped(_stack(['astronaut', 'rings']), n)
    plan = _plan(psfs, 2, n, n, dtype)
    plan.set_object(obj, 1e9)
    plan.simulate(seed=6)
    meas = plan.measurement()
    assert plan.strategy()['frame_pairs'] == (dtype == 'f32' and views == 1)
    plan.iterate(20)
    want = plan.estimate()
    plan.divergence()
    plan.iterate_until(11, rule=sr.RELATIVE, threshold=1e-2, check_every=3)
    plan.divergence()
    plan.set_measurement(meas)
    plan.reset_estimate()
    plan.iterate(20)
    assert np.array_equal(plan.estimate(), want)
