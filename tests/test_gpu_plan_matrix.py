"""Every loop a plan may choose, in every mode, against one numpy model of the plan (tests/plan_model.py) on the admitted cases of
tests/plan_cases.py: the scripted sequence of a case runs on the model and on an f64 and an f32 plan side by side, and every step
that changes the estimate is compared.  float64 plans: normwise 1e-10 per frame, pixelwise 1e-8, alpha within 1e-9, iterate_until's
counts and flags equal to the model's.  float32 plans: normwise 1e-5, no unresolved pixel.  The stencil rows also run
the case on an f64 plan of the FFT strategy.  Last: a plan with a history computes, bit for bit, what a fresh plan computes.

Measured on an MI355X (each test prints its largest errors, `-s`): f64 <= 1.1e-13 normwise, 2.5e-13 pixelwise; f32 <= 2.4e-6 on every
case but pair_b5 under BA + TV, 9.8e-6."""
import ctypes

import numpy as np
import pytest

import plan_cases as pc
import stop_reference as sr
from conftest import max_rel
from plan_model import PlanModel

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-10, 'f32': 1e-5}
PIXEL_F64, ALPHA_F64 = 1e-8, 1e-9


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


def _pixel_rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * np.max(np.abs(b)))))


def _frame_rel(a, b):
    return max(max_rel(a[f], b[f]) for f in range(b.shape[0]))


def _create(env, psfs, B, ny, nx, dtype, mode):
    """A plan created with the options `env`, in the mode `mode`."""
    acceleration, lam = pc.MODES[mode]
    return _lib().DeconvPlan(psfs, B, ny, nx, dtype=dtype, acceleration=acceleration, tv_lambda=lam, tv_epsilon=pc.TV_EPSILON, options=env)


_CHUNK_MB = {}


def _sliced(case, d, env, dtype, mode):
    """The slices row: the plan under the smallest RLSTED_CHUNK_MB that cuts its five frames into three slices (2, 2, 1), found once
    per element type and mode by asking the plan after a cycle (rl_deconv_object_classes)."""
    key = (dtype, mode)
    budgets = [_CHUNK_MB[key]] if key in _CHUNK_MB else list(0.03 * 1.15 ** np.arange(40))
    for mb in budgets:
        plan = _create(dict(env, RLSTED_CHUNK_MB='%.5f' % mb), d['psfs'], case['B'], case['ny'], case['nx'], dtype, mode)
        plan.set_object(d['obj'])
        plan.bench_cycles(1, 1)
        if plan.object_classes()['slices'] == 3:
            _CHUNK_MB[key] = mb
            return plan
    raise AssertionError('no RLSTED_CHUNK_MB gives three slices: %r' % (key,))


def _write_measurement(plan, dtype, m):
    """Straight into the plan's buffer (rl_device_upload at the address rl_deconv_device_ptr hands out), then measurement_written."""
    L = _lib()
    addr = plan.device_array('measurement').__cuda_array_interface__['data'][0]
    v = np.ascontiguousarray(m, dtype=np.float64)
    L.check(L.lib.rl_device_upload(plan.ctx.handle, ctypes.c_void_p(addr), L.DTYPES[dtype], v.size, L.ptr(v)))
    plan.measurement_written()


def _run_plan(plan, dtype, d, op):
    if op[0] == 'set_measurement':
        return plan.set_measurement(d['meas'][op[1]])
    if op[0] == 'written':
        return _write_measurement(plan, dtype, d['meas'][op[1]])
    if op[0] == 'keep_measurement':
        keep = plan.estimate()
        plan.set_measurement(d['meas'][op[1]])
        return plan.set_estimate(keep)
    if op[0] == 'iterate':
        return plan.iterate(op[1])
    if op[0] == 'forward':
        return plan.forward(d['obj'])
    if op[0] == 'adjoint':
        return plan.adjoint(d['meas'][0])
    if op[0] == 'divergence':
        return plan.divergence()
    if op[0] == 'mode':
        return pc.set_mode(plan, op[1])
    if op[0] == 'set_estimate':
        return plan.set_estimate(d['x'])
    if op[0] == 'until':
        return plan.iterate_until(op[1], rule=op[3], threshold=op[4], check_every=op[2])
    raise ValueError(op)


def _check_divergence(D, model, dtype, tag):
    """D against stop_reference.divergence on the MODEL's prediction: the order of the device's sum (summation_bound) plus what
    the plan's contract lets the prediction move (contract_bound at the element type's tolerance)."""
    pred = model.prediction()
    n_frame = model.V * model.ny * model.nx
    chain = sr.chain_length(n_frame, 4 if dtype == 'f32' else 8)
    for f in range(model.B):
        m = np.stack([v[f] for v in model.meas])
        want = sr.divergence(m, pred[f])
        bound = sr.summation_bound(m, pred[f], chain) + sr.contract_bound(m, pred[f], rel=TOL[dtype])
        if dtype == 'f32':                                   # the plan holds the measurement rounded to float32: dD/dm = log(m / p)
            bound += float(np.sum(np.abs(np.log(m / pred[f])) * np.abs(m - m.astype(np.float32).astype(np.float64))))
        assert abs(D[f] - want) <= bound, (tag, f, D[f], want, bound)


@pytest.mark.parametrize('mode', list(pc.MODES))
@pytest.mark.parametrize('name', [c['name'] for c in pc.CASES])
def test_sequence_follows_the_model(name, mode):
    case, d = pc.BY_NAME[name], pc.data(name)
    B, ny, nx = case['B'], case['ny'], case['nx']
    model = PlanModel(d['psfs'], B, ny, nx)
    pc.set_mode(model, mode)
    plans = {}
    for dtype in ('f64', 'f32'):
        env = dict(case['env'], **(case['env32'] if dtype == 'f32' else {}))
        make = _sliced if case['slices'] else (lambda c, dd, e, t, md: _create(e, dd['psfs'], B, ny, nx, t, md))
        plans[dtype] = make(case, d, env, dtype, mode)
    if case['twin'] is not None:                             # the same f64 case on another strategy
        plans['twin'] = _create(dict(case['env'], **case['twin']), d['psfs'], B, ny, nx, 'f64', mode)

    def check_strategy(expect_pairs=None):
        for key, plan in plans.items():
            strat, want = plan.strategy(), case['want32' if key == 'f32' else 'want64']
            if key == 'twin':
                want = {'separable': False} if case['row'] == 'separable' else {'direct_stencil': False}
            for k, v in want.items():
                assert strat[k] == v, (name, key, strat)
            if case['lengths'] and key != 'twin':
                info = plan.info()
                assert (info['ly'], info['lx']) == case['lengths'], (name, key, info)
            if expect_pairs is not None:
                assert strat['frame_pairs'] == (expect_pairs and key == 'f32'), (name, key, strat)
    check_strategy()
    worst = {k: 0.0 for k in plans}
    pixel = 0.0
    accel_on = pc.MODES[mode][0] is not None
    for step, op in enumerate(pc.script(case, mode)):
        want = pc.run_model(model, d, op)
        if op[0] == 'mode':
            accel_on = pc.MODES[op[1]][0] is not None
        for key, plan in plans.items():
            dtype = 'f32' if key == 'f32' else 'f64'
            tag = (name, mode, key, step, op)
            got = _run_plan(plan, dtype, d, op)
            if op[0] in ('set_measurement', 'keep_measurement') and case['row'] == 'pair_switch':
                lv = case['levels'][op[1]]                   # the loop follows the partners' levels: within a factor of 4 or not
                pairs = all(max(lv[f], lv[f + 1]) <= 3.5 * min(lv[f], lv[f + 1]) for f in range(0, B - 1, 2))
                assert plan.strategy()['frame_pairs'] == (pairs and key == 'f32'), tag
            if op[0] in ('forward', 'adjoint'):
                err = max_rel(got, want)
                assert err <= TOL[dtype], (tag, err)
            elif op[0] == 'divergence':
                _check_divergence(got, model, dtype, tag)
            if op[0] not in ('iterate', 'until'):
                continue
            est, ref = plan.estimate(), model.est
            if op[0] == 'until':                             # every frame against the model at the check the plan kept
                its = got['iterations']
                if dtype == 'f64':
                    assert np.array_equal(its, want['iterations']), (tag, got, want)
                    assert np.array_equal(got['stopped'], want['stopped']), (tag, got, want)
                assert all(int(k) in want['estimates'] for k in its), (tag, got)
                ref = np.stack([want['estimates'][int(its[f])][f] for f in range(B)])
                if np.array_equal(its, want['iterations']):
                    _check_divergence(got['divergence'], model, dtype, tag)
            err = _frame_rel(est, ref) if dtype == 'f64' else max_rel(est, ref)
            worst[key] = max(worst[key], err)
            assert err <= TOL[dtype], (tag, err)
            if dtype == 'f64':
                pixel = max(pixel, _pixel_rel(est, ref))
                assert _pixel_rel(est, ref) <= PIXEL_F64, (tag, _pixel_rel(est, ref))
                if accel_on and op[0] == 'iterate':
                    assert np.max(np.abs(plan.alpha() - model.alpha())) <= ALPHA_F64, (tag, plan.alpha(), model.alpha())
        if op[0] == 'iterate' and 'twin' in plans:           # stencil and FFT strategy of the same f64 case
            err = _frame_rel(plans['f64'].estimate(), plans['twin'].estimate())
            assert err <= 1e-10, (name, mode, step, op, err)
    if case['row'] in ('pair', 'pair_switch'):
        check_strategy(expect_pairs=True)                    # (the last measurement's partners are of comparable level)
    assert plans['f32'].unresolved() == 0
    print('PLANMATRIX %s %s %s f64 %.3e pixel %.3e f32 %.3e%s' % (case['row'], name, mode, worst['f64'], pixel, worst['f32'],
                                                               ' twin %.3e' % worst['twin'] if 'twin' in worst else ''))


# ---------------------------------------------------------------------------------------------- a plan with a history == a fresh plan
def _negative(m):
    out = np.array(m, dtype=np.float64, copy=True)
    out[..., ::7, ::5] -= 2.0 * np.abs(out[..., ::7, ::5]) + 1.0          # background-subtracted data: some pixels below zero
    assert (out < 0).any()
    return out


def _device_buffer(plan, n, dtype):
    L = _lib()
    dev = ctypes.c_void_p()
    L.check(L.lib.rl_device_alloc(plan.ctx.handle, n * (4 if dtype == 'f32' else 8), ctypes.byref(dev)))
    return dev


def _download(plan, dev, n, dtype):
    L = _lib()
    plan.ctx.synchronize()
    out = np.empty(n)
    L.check(L.lib.rl_device_download(plan.ctx.handle, dev, L.DTYPES[dtype], n, L.ptr(out)))
    L.check(L.lib.rl_device_free(plan.ctx.handle, dev))
    return out


@pytest.mark.parametrize('last', ['simulate', 'set_measurement', 'batch_submit', 'bench_cycles'])
@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_plan_with_a_history_equals_a_fresh_plan(dtype, views, last):
    """After any prefix of calls -- a mode set and unset, a measurement with negative pixels (a multi-view f32 plan then leaves its
    `ratio - 1` arithmetic), the pair choice flipped, D, a set estimate -- the last two calls give the bits a fresh plan gives."""
    name = 'switch_b4' if views == 1 else 'views3'
    case, d = pc.BY_NAME[name], pc.data(name)
    B, ny, nx, K = case['B'], case['ny'], case['nx'], 5
    n = B * ny * nx

    def finish(plan):
        if last == 'simulate':
            plan.set_object(d['obj'])
            plan.simulate(seed=3)
            plan.iterate(K)
        elif last == 'set_measurement':
            plan.set_measurement(d['meas'][2])
            plan.iterate(K)
        elif last == 'bench_cycles':
            plan.set_object(d['obj'])
            plan.bench_cycles(K, 2, seed=3)
        else:
            dev = _device_buffer(plan, n, dtype)
            plan.batch_submit(list(d['obj']), None, 3, list(range(B)), K, dev, out_dtype=dtype)
            return _download(plan, dev, n, dtype).reshape(B, ny, nx), plan.strategy()
        return plan.estimate(), plan.strategy()

    used = _create(case['env'], d['psfs'], B, ny, nx, dtype, 'batv')
    pc.set_mode(used, 'plain')
    used.set_measurement(_negative(d['meas'][0]))
    used.iterate(2)
    if views == 1:
        used.set_measurement(d['meas'][1])                                  # partners beyond a factor of 4: the per-frame loop
        assert not used.strategy()['frame_pairs']
        used.iterate(4)
    used.divergence()
    used.set_estimate(d['x'])
    used.iterate(1)
    got, strat = finish(used)
    fresh = _create(case['env'], d['psfs'], B, ny, nx, dtype, 'plain')
    want, strat_fresh = finish(fresh)
    assert strat == strat_fresh
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want), (dtype, views, last, max_rel(got, want))
