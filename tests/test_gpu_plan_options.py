"""The switches of a plan as an argument (rl_deconv_create_with, DeconvPlan(options=...)): the text gives what the environment
gives, wins over it, lets two plans of one process differ, and is refused when it names something that is no switch of a plan.
The table itself -- defaults, clamps, parsing -- is tested on the CPU (tests/test_plan_options_cpu.py); the other GPU tests
create their plans through options, so this file is the one place that keeps the environment's way in under test."""
import ctypes
import os

import numpy as np
import pytest

import plan_cases as pc
from conftest import max_rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['slices_lane1', 'sep_two_pass', 'split_v3'])
def test_options_equal_the_environment(lib, monkeypatch, name, dtype):
    """Rows of the plan matrix: five frames of 40 x 36 on the FFT path with one lane, the two-pass stencils at 45 x 61 with 7 x 5
    taps, the split column pass (f32) of three views at column length 2304.  The case's dict as options and the same dict in the
    environment: the same strategy and, after the same cycle on the same object, the same bits."""
    case, d = pc.BY_NAME[name], pc.data(name)
    options = dict(case['env'], **(case['env32'] if dtype == 'f32' else {}))
    assert options
    args = (d['psfs'], case['B'], case['ny'], case['nx'])
    given = lib.DeconvPlan(*args, dtype=dtype, options=options)
    with monkeypatch.context() as mp:
        for k, v in options.items():
            mp.setenv(k, v)
        from_env = lib.DeconvPlan(*args, dtype=dtype)
    want = case['want32' if dtype == 'f32' else 'want64']
    assert {k: given.strategy()[k] for k in want} == want
    assert given.strategy() == from_env.strategy()
    for plan in (given, from_env):
        plan.set_object(d['obj'])
        plan.bench_cycles(3, 1, seed=7)
    assert np.array_equal(given.measurement(), from_env.measurement())
    assert np.array_equal(given.estimate(), from_env.estimate())
    assert given.object_classes() == from_env.object_classes()


def test_options_beat_the_environment_and_plans_differ_side_by_side(lib, monkeypatch):
    """RLSTED_SEP=0 in the environment: a plan given RLSTED_SEP=2 runs the stencils, a plan created right after it without options
    the FFT path.  Both stay alive and iterate in turns; their estimates agree as the two strategies do in
    tests/test_gpu_separable.py (float64, 20 iterations: 1e-11).  Neither constructor touches os.environ."""
    case, d = pc.BY_NAME['sep_two_pass'], pc.data('sep_two_pass')
    B, ny, nx = case['B'], case['ny'], case['nx']
    monkeypatch.setenv('RLSTED_SEP', '0')
    before = dict(os.environ)
    sep = lib.DeconvPlan(d['psfs'], B, ny, nx, dtype='f64', options={'RLSTED_SEP': '2'})
    fft = lib.DeconvPlan(d['psfs'], B, ny, nx, dtype='f64')
    assert dict(os.environ) == before
    assert sep.options == {'RLSTED_SEP': '2'} and fft.options == {}
    assert sep.strategy()['separable'] and not fft.strategy()['separable'] and not fft.strategy()['direct_stencil']
    obj = np.random.default_rng(11).random((B, ny, nx)) * 50
    for p in (sep, fft):
        p.set_object(obj, 1e7)
        p.simulate(seed=9)
    assert np.array_equal(sep.measurement(), fft.measurement())
    for _ in range(5):
        sep.iterate(4)
        fft.iterate(4)
    assert sep.strategy()['separable'] and not fft.strategy()['separable']
    assert max_rel(sep.estimate(), fft.estimate()) < 1e-11


@pytest.mark.parametrize('options, offender', [
    ({'RLSTED_LANE': '1'}, 'RLSTED_LANE'),                       # a misspelt switch
    ({'PAIR': '0'}, 'PAIR'),
    ('RLSTED_LANES=1 RLSTED_PAIR', 'RLSTED_PAIR'),               # no '='
    ('RLSTED_PAIR=0 RLSTED_LANES=1 RLSTED_PAIR=1', 'RLSTED_PAIR'),   # twice
])
def test_bad_options_are_refused(lib, options, offender):
    psfs = [np.random.default_rng(2).random((1, 5, 7)) + 0.05]
    with pytest.raises(lib.RlstedError) as err:
        lib.DeconvPlan(psfs, 2, 40, 36, dtype='f32', options=options)
    assert "'%s'" % offender in str(err.value), str(err.value)
    # no plan is left behind: the C call itself hands back a NULL handle and RL_ERR_INVALID (-1)
    ctx = lib.Context.get(0, 0)
    stack = lib.as_f64(np.concatenate(psfs, axis=0))
    handle = ctypes.c_void_p()
    text = options if isinstance(options, str) else ' '.join('%s=%s' % kv for kv in options.items())
    rc = lib.lib.rl_deconv_create_with(ctx.handle, lib.ptr(stack), 1, 5, 7, 2, 40, 36, lib.DTYPES['f32'], text.encode(), ctypes.byref(handle))
    assert rc == -1 and not handle.value
    assert "'%s'" % offender in lib.lib.rl_last_error().decode()
    # ... and a valid create right after it succeeds
    plan = lib.DeconvPlan(psfs, 2, 40, 36, dtype='f32', options={'RLSTED_LANES': '1', 'RLSTED_PAIR': '0'})
    x = np.ones((2, 40, 36))
    assert np.isfinite(plan.forward(x)).all() and not plan.strategy()['frame_pairs']
