"""The numpy model of a plan (tests/plan_model.py) and the cases of the plan matrix (tests/plan_cases.py), without a GPU: the model
adds no arithmetic to the oracle and the reference classes, its operators are the oracle's direct sum, every committed case is
admitted, and the matrix is complete."""
import numpy as np
import pytest

import plan_cases as pc
import stop_reference as sr
from accel_reference import AcceleratedRL
from conftest import max_rel
from oracle import line_sted_oracle as orc
from plan_model import BA, PlanModel
from tv_reference import AcceleratedRegularisedRL, RegularisedRL

TINY = ['pf_64', 'views2_even', 'direct_2x2']
NAMES = [c['name'] for c in pc.CASES]


def _model(name, mode):
    case, d = pc.BY_NAME[name], pc.data(name)
    acceleration, lam = pc.MODES[mode]
    model = PlanModel(d['psfs'], case['B'], case['ny'], case['nx'], acceleration=acceleration, tv_lambda=lam, tv_epsilon=pc.TV_EPSILON)
    model.set_measurement(d['meas'][0])
    return model, d


def _views(m):
    return [np.ascontiguousarray(m[:, v]) for v in range(m.shape[1])]


# ---------------------------------------------------------------------------------------------- 1. no arithmetic of its own
@pytest.mark.parametrize('name', TINY[:2])
def test_no_mode_is_the_oracles_iteration_bit_for_bit(name):
    model, d = _model(name, 'plain')
    o = orc.Deconvolver(d['psfs'])
    o.noisy_measurement = _views(d['meas'][0])
    for _ in range(6):
        o.iterate()
    model.iterate(6)
    assert np.array_equal(model.estimate(), o.estimate)
    assert np.all(model.alpha() == 0)


@pytest.mark.parametrize('mode', ['ba', 'tv', 'batv'])
@pytest.mark.parametrize('name', TINY[:2])
def test_each_mode_is_its_reference_class_bit_for_bit(name, mode):
    model, d = _model(name, mode)
    noisy = _views(d['meas'][0])
    ref = {'ba': lambda: AcceleratedRL(d['psfs'], noisy),
           'tv': lambda: RegularisedRL(d['psfs'], noisy, pc.TV_LAMBDA, pc.TV_EPSILON),
           'batv': lambda: AcceleratedRegularisedRL(d['psfs'], noisy, pc.TV_LAMBDA, pc.TV_EPSILON)}[mode]()
    ref.iterate(7)
    model.iterate(7)
    assert np.array_equal(model.estimate(), ref.estimate)
    if mode != 'tv':
        assert np.array_equal(model.alpha(), ref.alpha) and np.all(ref.alpha > 0)
    # ... and from a set estimate, on new data
    ref.set_measurement(_views(d['meas'][1]))
    ref.set_estimate(d['x'])
    ref.iterate(3)
    model.set_measurement(d['meas'][1])
    model.set_estimate(d['x'])
    model.iterate(3)
    assert np.array_equal(model.estimate(), ref.estimate)


@pytest.mark.parametrize('mode', list(pc.MODES))
def test_any_split_gives_the_bits_of_one_run(mode):
    whole, d = _model('pf_64', mode)
    whole.iterate(7)
    for split in ((1, 6), (3, 1, 3), (2, 0, 5), (1, 1, 1, 1, 1, 1, 1)):
        model, _ = _model('pf_64', mode)
        for k in split:
            model.iterate(k)
            model.forward(d['obj'])                     # the operators and D leave the estimate and the history alone
            model.adjoint(d['meas'][0])
            model.divergence()
        assert np.array_equal(model.estimate(), whole.estimate()), (mode, split)
        assert np.array_equal(model.alpha(), whole.alpha())


def test_state_rules_between_the_references():
    model, d = _model('pf_64', 'ba')
    noisy = _views(d['meas'][0])
    model.iterate(4)
    x4 = model.estimate()
    # a change of mode restarts the history, the estimate stays: plain steps from x4, then accelerated steps with a = 0 first
    model.set_acceleration(None)
    model.iterate(2)
    plain = RegularisedRL(d['psfs'], noisy, lam=0.0)
    plain.set_estimate(x4)
    plain.iterate(2)
    assert np.array_equal(model.estimate(), plain.estimate)
    model.set_acceleration(BA)
    model.iterate(3)
    ref = AcceleratedRL(d['psfs'], noisy)
    ref.set_estimate(plain.estimate)
    ref.iterate(3)
    assert np.array_equal(model.estimate(), ref.estimate) and np.array_equal(model.alpha(), ref.alpha)
    # the same mode set again is no change: the history goes on
    model.set_acceleration(BA)
    model.iterate(1)
    ref.iterate(1)
    assert np.array_equal(model.estimate(), ref.estimate)
    # set_tv takes effect from the next iterate and leaves the history alone
    model.set_tv(pc.TV_LAMBDA, pc.TV_EPSILON)
    model.iterate(2)
    tv = AcceleratedRegularisedRL(d['psfs'], noisy, pc.TV_LAMBDA, pc.TV_EPSILON)
    tv.set_estimate(ref.estimate)
    tv.x_prev, tv.g_prev, tv.next_alpha, tv.steps = ref.x_prev, ref.g_prev, ref.next_alpha, ref.steps
    tv.iterate(2)
    assert np.array_equal(model.estimate(), tv.estimate)
    # new data and reset_estimate start from ones; measurement_written is set_measurement
    model.measurement_written(d['meas'][2])
    model.iterate(2)
    tv.set_measurement(_views(d['meas'][2]))
    tv.iterate(2)
    assert np.array_equal(model.estimate(), tv.estimate)
    model.reset_estimate()
    model.iterate(2)
    assert np.array_equal(model.estimate(), tv.estimate)


def test_iterate_until_is_the_stepwise_sequence():
    model, d = _model('views2_even', 'plain')
    t_rel, _ = pc.THRESHOLDS[('views2_even', 'plain')]
    model.set_estimate(d['x'])
    info = model.iterate_until(3, rule=sr.RELATIVE, threshold=t_rel, check_every=1)
    step, _ = _model('views2_even', 'plain')
    step.set_estimate(d['x'])
    N = step.V * step.ny * step.nx
    prev, kept = None, {}
    for k in (1, 2, 3):
        step.iterate(1)
        D = step.divergence()
        for f in range(step.B):
            if f not in kept and (sr.rule_met(sr.RELATIVE, t_rel, N, D[f], None if prev is None else prev[f]) or k == 3):
                kept[f] = (k, D[f], step.estimate()[f])
        prev = D
    assert sorted(set(info['iterations'])) == [2, 3]             # (the threshold separates the frames)
    for f in range(step.B):
        assert info['iterations'][f] == kept[f][0] and info['divergence'][f] == kept[f][1]
        assert np.array_equal(model.estimate()[f], kept[f][2])
    assert info['stopped'][info['iterations'] == 2].all()     # (a frame kept before the last check met the rule)


# ---------------------------------------------------------------------------------------------- 2. the operators
@pytest.mark.parametrize('name', TINY)
def test_operators_are_the_direct_sum(name):
    model, d = _model(name, 'plain')
    h = model.forward(d['obj'])
    for v, p in enumerate(d['psfs']):
        assert max_rel(h[:, v], np.maximum(orc.conv_same_direct(d['obj'], p), 0)) <= 1e-13
    y = d['meas'][0]
    want = sum(np.maximum(orc.conv_same_direct(y[:, v], p), 0) for v, p in enumerate(d['psfs']))
    norm = sum(np.maximum(orc.conv_same_direct(np.ones_like(y[:, v]), p), 0) for v, p in enumerate(d['psfs']))
    assert max_rel(model.adjoint(y, normalize=False), want) <= 1e-13
    assert max_rel(model.adjoint(y), want / norm) <= 1e-13


# ---------------------------------------------------------------------------------------------- 3. admission
@pytest.mark.parametrize('name', NAMES)
def test_every_committed_case_is_admitted(name):
    for mode in pc.MODES:
        fig = pc.admit(name, mode)
        print(name, mode, fig)
        assert fig['finite'], (name, mode)
        assert fig['min_ratio'] >= pc.MIN_PREDICTION_RATIO, (name, mode, fig)
        assert fig['sensitivity'] <= pc.F32_SENSITIVITY, (name, mode, fig)
        assert fig['margin'] >= pc.THRESHOLD_MARGIN, (name, mode, fig)


# ---------------------------------------------------------------------------------------------- 4. the matrix is complete
def test_the_matrix_is_complete():
    rows = {r: [c for c in pc.CASES if c['row'] == r] for r in pc.ROWS}
    assert all(rows[r] for r in pc.ROWS) and sum(len(v) for v in rows.values()) == len(pc.CASES)
    assert set(pc.THRESHOLDS) == {(c['name'], m) for c in pc.CASES for m in pc.MODES}     # every case runs every mode, f64 and f32
    assert {c['lengths'] for c in rows['per_frame']} == {(64, 64), (192, 64), (256, 64), (576, 64), (64, 1152)}
    assert all(c['psf'][1] == 1 and c['env32'] == {'RLSTED_PAIR': '0'} for c in rows['per_frame'])
    assert {c['B'] for c in rows['pair']} == {2, 3, 5} and all((c['ny'], c['nx']) == (200, 200) for c in rows['pair'])
    assert any(c['written'] for c in pc.CASES)
    (sw,) = rows['pair_switch']
    within = [all(max(lv[f], lv[f + 1]) <= 4 * min(lv[f], lv[f + 1]) for f in (0, 2)) for lv in sw['levels']]
    assert sw['B'] == 4 and within == [True, False, True]
    assert {c['psf'][1] for c in rows['multi_view']} == {2, 3, 4}
    assert any(c['psf'][2] % 2 == 0 or c['psf'][3] % 2 == 0 for c in rows['multi_view'])
    assert {c['psf'][1] for c in rows['split']} == {2, 3} and all((c['ny'], c['nx']) == (1153, 40) for c in rows['split'])
    assert {c['env'].get('RLSTED_SEP_ONE') for c in rows['separable']} == {'0', '1'}
    assert all(c['psf'][2] + c['psf'][3] <= 16 and max(c['ny'], c['nx']) <= 64 and c['twin'] for c in rows['separable'])
    assert all(2 <= min(c['psf'][2:]) and max(c['psf'][2:]) <= 7 and max(c['ny'], c['nx']) <= 64 and c['twin'] for c in rows['direct'])
    assert {c['env'].get('RLSTED_LANES') for c in rows['slices']} == {'1', '2'} and all(c['B'] == 5 and c['slices'] for c in rows['slices'])
    for c in pc.CASES:                                       # the sequence every case runs
        ops = pc.script(c, 'plain')
        counts = [op[1] for op in ops if op[0] in ('iterate', 'until')]
        assert sum(counts) <= 12 and any(1 <= k <= 3 for k in counts) and any(k >= 4 for k in counts)
        kinds = [op[0] for op in ops]
        for kind in ('forward', 'adjoint', 'divergence', 'set_estimate', 'mode', 'keep_measurement'):
            assert kind in kinds
        assert {op[2] for op in ops if op[0] == 'until'} == {1, 3}
