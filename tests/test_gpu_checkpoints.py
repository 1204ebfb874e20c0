"""Iteration checkpoints of the enqueued sweep (include/rlsted.h rl_batch_submit_checkpoints; rlsted.cpp run_slices,
csrc/checkpoint_kernels.hpp).  Needs an MI355X.

The core check is bit equality: checkpoint j of a run with k_list is what rl_batch_submit with k_list[j] writes for the same tasks on
a fresh plan of the same options -- np.array_equal, no tolerance -- on every loop the plan can run.  The trace is held to the bound
derived in tests/checkpoint_reference.py against numpy long double sums of the downloaded checkpoint and the plan's object.
"""
import ctypes

import numpy as np
import pytest

import checkpoint_reference as cr

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8]
SENTINEL = -777.0
RL_ERR_INVALID = -1


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def gauss(n, s, shift=0.0):
    x = np.arange(n) - (n - 1) / 2.0 - shift
    g = np.exp(-0.5 * (x / s) ** 2)
    return g / g.sum()


def random_psfs(V, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.random((1, 9, 9)) + 0.05 for _ in range(V)]


def make_objects(pattern, ny, nx, seed=11):
    rng = np.random.default_rng(seed)
    kinds = {c: rng.random((ny, nx)) * 200 + 1 for c in sorted(set(pattern))}
    return [kinds[c] for c in pattern]


class Buffer:
    """A float64 or float32 device buffer of `count` elements, filled with the sentinel."""

    def __init__(self, count, dtype):
        from rescan_line_sted_amd import sweep
        self.res = sweep.DeviceResults.from_host([np.full((1, count), SENTINEL)], dtype)

    @property
    def address(self):
        return self.res.dev.value

    def download(self):
        return self.res.download()[0].ravel()

    def free(self):
        self.res.free()


# name: (psfs, dtype, ny, nx, batch, object pattern = the tasks, plan keywords, the plan's options, strategy to expect)
CASES = {
    'f64_two_chunks_short_last': (random_psfs(1), 'f64', 48, 40, 5, 'ABCABCA', {}, {}, {'frame_pairs': False, 'separable': False}),
    # (no plan of 128 x 128 or less pairs its frames: the pair loop exists on the transforms from L = 256 on, and 200 x 200 is the size
    # the other tests take for it)
    'f32_frame_pairs': (random_psfs(1), 'f32', 200, 200, 6, 'ABCABC', {}, {}, {'frame_pairs': True}),
    'f32_three_views': (random_psfs(3), 'f32', 48, 40, 4, 'ABAB', {}, {}, {'frame_pairs': False, 'separable': False}),
    'rank1_separable': ([np.outer(gauss(7, 1.0), gauss(5, 2.0))[None]], 'f32', 64, 64, 4, 'ABCA', {}, {}, {'separable': True}),
    'direct_stencil': ([(np.outer(gauss(5, 1.2), gauss(5, 1.2)) + np.eye(5) * 0.01)[None]], 'f64', 64, 64, 4, 'ABCA', {}, {},
                       {'direct_stencil': True, 'separable': False}),
    'biggs_andrews': (random_psfs(1), 'f32', 48, 40, 4, 'ABCA', {'acceleration': 'biggs-andrews'}, {}, {}),
    'biggs_andrews_f64': (random_psfs(2), 'f64', 48, 40, 3, 'ABCA', {'acceleration': 'biggs-andrews'}, {}, {}),
    'tv': (random_psfs(1), 'f32', 48, 40, 4, 'ABCA', {'tv_lambda': 0.01}, {}, {}),
    'tv_f64': (random_psfs(2), 'f64', 48, 40, 3, 'ABCA', {'tv_lambda': 0.01}, {}, {}),
    'slices_on_two_lanes_shared_classes': (random_psfs(1), 'f64', 128, 128, 12, 'ABCDAAAAEEFF', {}, {'RLSTED_CHUNK_MB': '2.0', 'RLSTED_LANES': '2'},
                                           {'separable': False}),
}


def make_plan(lib, case, batch=None):
    psfs, dtype, ny, nx, B, _, kw, options, want = CASES[case]
    plan = lib.DeconvPlan(psfs, batch or B, ny, nx, dtype=dtype, options=options, **kw)
    s = plan.strategy()
    if batch is None:
        assert {k: s[k] for k in want} == want, (case, s)
    return plan


def tasks_of(case, brightness=3e6):
    _, _, ny, nx, _, pattern, _, _, _ = CASES[case]
    objs = make_objects(pattern, ny, nx)
    n = len(objs)
    ids = [ord(c) - ord('A') for c in pattern]
    seeds = [100 + t // 2 for t in range(n)]
    return objs, brightness, seeds, ids


def plain(lib, case, K, out_dtype, slots=None):
    """rl_batch_submit with K iterations on a fresh plan: the downloaded buffer [slots][ny][nx] (sentinel behind the tasks)."""
    _, _, ny, nx, _, pattern, _, _, _ = CASES[case]
    objs, tb, seeds, ids = tasks_of(case)
    plan = make_plan(lib, case)
    buf = Buffer((slots or len(objs)) * ny * nx, out_dtype)
    plan.batch_submit(objs, tb, seeds, ids, K, buf.address, out_dtype)
    plan.ctx.synchronize()
    out = buf.download().reshape(-1, ny, nx)
    buf.free()
    return out, plan


def checkpoints(lib, case, ks, out_dtype, outs=True, traces=True, slots=None, skip=(), plan=None, select=None):
    """rl_batch_submit_checkpoints on a fresh plan (or `plan`): ([n_k] downloaded buffers or None, [n_k][slots][6] traces or None,
    the plan).  Checkpoints listed in `skip` get NULL entries in both arrays; `select`: the indices of the case's tasks to run."""
    _, _, ny, nx, _, pattern, _, _, _ = CASES[case]
    objs, tb, seeds, ids = tasks_of(case)
    if select is not None:
        objs, seeds, ids = [objs[i] for i in select], [seeds[i] for i in select], [ids[i] for i in select]
    plan = plan or make_plan(lib, case)
    slots = slots or len(objs)
    obufs = [Buffer(slots * ny * nx, out_dtype) for _ in ks] if outs else None
    tbufs = [Buffer(slots * cr.FIELDS, 'f64') for _ in ks] if traces else None

    def addresses(bufs):
        return None if bufs is None else [None if j in skip else b.address for j, b in enumerate(bufs)]
    plan.batch_submit_checkpoints(objs, tb, seeds, ids, ks, addresses(obufs), out_dtype, addresses(tbufs))
    plan.ctx.synchronize()
    est = [b.download().reshape(-1, ny, nx) for b in obufs] if outs else None
    tr = np.stack([b.download().reshape(-1, cr.FIELDS) for b in tbufs]) if traces else None
    for b in (obufs or []) + (tbufs or []):
        b.free()
    return est, tr, plan


# ------------------------------------------------------------------ bit equality with separate runs
@pytest.mark.parametrize('case', sorted(CASES))
def test_checkpoints_are_the_separate_runs(lib, case):
    _, dtype, ny, nx, B, pattern, _, _, _ = CASES[case]
    n = len(pattern)
    slots = n + 3
    est, tr, plan = checkpoints(lib, case, KS, dtype, slots=slots)
    if case == 'slices_on_two_lanes_shared_classes':
        assert plan.object_classes() == {'classes': 6, 'shared_slices': 2, 'slices': 3}
    for j, K in enumerate(KS):
        want, _ = plain(lib, case, K, dtype, slots=slots)
        assert np.all(want[n:] == SENTINEL) and np.all(want[:n] != SENTINEL)
        assert np.array_equal(est[j], want), (case, K)                 # (the untouched slots behind the tasks included)
        assert np.all(tr[j, n:] == SENTINEL) and np.all(np.isfinite(tr[j, :n]))
    # the plan is left as the plain run with the last count leaves it
    _, plan_k = plain(lib, case, KS[-1], dtype)
    assert np.array_equal(plan.estimate(), plan_k.estimate())
    assert np.array_equal(plan.measurement(), plan_k.measurement())


@pytest.mark.parametrize('case,out_dtype', [('f64_two_chunks_short_last', 'f32'), ('f32_frame_pairs', 'f64')])
def test_a_destination_of_the_other_type(lib, case, out_dtype):
    n = len(CASES[case][5])
    est, _, _ = checkpoints(lib, case, [2, 5], out_dtype, traces=False, slots=n + 1)
    for j, K in enumerate([2, 5]):
        want, _ = plain(lib, case, K, out_dtype, slots=n + 1)
        assert np.array_equal(est[j], want), (case, K)


# ------------------------------------------------------------------ calls that must agree
@pytest.mark.parametrize('case', ['f64_two_chunks_short_last', 'f32_frame_pairs'])
def test_calls_that_must_agree(lib, case):
    dtype = CASES[case][1]
    full_e, full_t, _ = checkpoints(lib, case, KS, dtype)
    # one checkpoint at K is the plain run
    one_e, one_t, _ = checkpoints(lib, case, [5], dtype)
    want, plan_k = plain(lib, case, 5, dtype)
    assert np.array_equal(one_e[0], want) and np.array_equal(one_e[0], full_e[3]) and np.array_equal(one_t[0], full_t[3])
    # NULL entries inside the arrays change nothing else
    e2, t2, _ = checkpoints(lib, case, KS, dtype, skip=(1, 4))
    for j in range(len(KS)):
        if j in (1, 4):
            assert np.all(e2[j] == SENTINEL) and np.all(t2[j] == SENTINEL)
        else:
            assert np.array_equal(e2[j], full_e[j]) and np.array_equal(t2[j], full_t[j])
    # estimates only, traces only: the same bits; with trace_dev only the plan's final estimate is the plain run's
    e3, _, _ = checkpoints(lib, case, KS, dtype, traces=False)
    _, t4, plan4 = checkpoints(lib, case, KS, dtype, outs=False)
    assert all(np.array_equal(a, b) for a, b in zip(e3, full_e)) and np.array_equal(t4, full_t)
    _, plan8 = plain(lib, case, KS[-1], dtype)
    assert np.array_equal(plan4.estimate(), plan8.estimate())
    # a second call on the same plan: the same bits again
    _, t5, _ = checkpoints(lib, case, KS, dtype, outs=False, plan=plan4)
    assert np.array_equal(t5, full_t)


# ------------------------------------------------------------------ trace parity
@pytest.mark.parametrize('case', ['f64_two_chunks_short_last', 'f32_frame_pairs', 'slices_on_two_lanes_shared_classes'])
def test_trace_against_long_double(lib, case):
    """A single-chunk run (the plan's batch covers the tasks): every field of every checkpoint of every task within the derived
    bound of the long double sums of the downloaded checkpoint and the plan's object; the same bits from a second run."""
    _, dtype, ny, nx, B, pattern, _, _, _ = CASES[case]
    select = list(range(min(B, len(pattern))))
    est, tr, plan = checkpoints(lib, case, KS, dtype, select=select)
    obj = plan.object()
    esize = 4 if dtype == 'f32' else 8
    worst = 0.0
    for j, K in enumerate(KS):
        for t in range(len(select)):
            worst = max(worst, cr.check(tr[j, t], est[j][t], obj[t], esize, '%s K=%d task %d' % (case, K, t)))
    print('%s: worst error / bound %.3g' % (case, worst))
    # semi-convergence is a property of the data; the sums of T are the same at every checkpoint
    assert np.array_equal(tr[0, :, [1, 3]], tr[-1, :, [1, 3]])
    est2, tr2, _ = checkpoints(lib, case, KS, dtype, select=select)
    assert np.array_equal(tr2, tr) and all(np.array_equal(a, b) for a, b in zip(est, est2))


def test_trace_of_a_task_alone_and_in_a_batch(lib):
    """f64: a task's estimate does not depend on its place in the list, and its trace is a function of estimate and object only --
    task 5 of the two-chunk batch (the second chunk's first) gives the bits it gives alone in a plan of one frame."""
    case = 'f64_two_chunks_short_last'
    est, tr, _ = checkpoints(lib, case, KS, 'f64')
    alone = make_plan(lib, case, batch=1)
    e1, t1, _ = checkpoints(lib, case, KS, 'f64', plan=alone, select=[5])
    for j in range(len(KS)):
        assert np.array_equal(e1[j][0], est[j][5]) and np.array_equal(t1[j, 0], tr[j, 5]), KS[j]


# ------------------------------------------------------------------ the Python layer
@pytest.fixture(scope='module')
def small_sweep():
    rng = np.random.default_rng(8)
    objects = {'a': rng.random((64, 64)) * 50 + 1, 'b': np.outer(np.hanning(64), np.hanning(64)) * 80 + rng.random((64, 64))}
    psf_sets = {'one': random_psfs(1, seed=5), 'two': random_psfs(2, seed=6)}
    return objects, psf_sets


def test_run_tasks_checkpoints_device(lib, small_sweep):
    from rescan_line_sted_amd import quality, sweep
    objects, psf_sets = small_sweep
    tasks = sweep.make_tasks(objects, psf_sets, (3, 4, 5))
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    ks = [1, 3, 6]
    results, trace = sweep.run_tasks_checkpoints_device(tasks, objects, psf_sets, ks, total_brightness=1e6)
    assert len(results) == 3 and trace.shape == (3, 12, quality.TRACE_FIELDS) and np.all(np.isfinite(trace))
    for j, K in enumerate(ks):
        res = sweep.run_tasks_device(tasks, objects, psf_sets, K, total_brightness=1e6)
        a, b = results[j].download(), res.download()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), K
        res.free()
    none, trace_only = sweep.run_tasks_checkpoints_device(tasks, objects, psf_sets, ks, total_brightness=1e6, estimates=False)
    assert none is None and np.array_equal(trace_only, trace)
    only, no_trace = sweep.run_tasks_checkpoints_device(tasks, objects, psf_sets, ks, total_brightness=1e6, trace=False)
    assert no_trace is None and all(np.array_equal(x, y) for x, y in zip(only[2].download(), results[2].download()))
    # the trace against the estimates it was taken from, f32 plans: T is the scaled object rounded to float32
    est = results[1].download()
    for t, (o, _, _) in enumerate(tasks):
        T = (objects[o] * (1e6 / objects[o].sum())).astype(np.float32).astype(np.float64)
        ref = cr.sums(est[t], T)
        assert np.allclose(trace[1, t].astype(np.float64), ref.astype(np.float64), rtol=1e-5)   # (T to the rounding of the device's scaling)
        assert abs(float(trace[1, t, 0] - ref[0])) <= cr.bounds(est[t], T, 4)[0]                   # sum x involves no T
    m = quality.trace_metrics(trace, 64 * 64)
    assert np.all((m['ncc'] > 0) & (m['ncc'] <= 1)) and np.all(np.abs(m['flux'] - 1) < 0.05)        # (object 'a' is white noise: a low correlation)
    for r in results + only:
        r.free()


def test_bias_variance_vs_iterations_is_the_old_loop(lib, small_sweep):
    from rescan_line_sted_amd import sweep
    objects, psf_sets = small_sweep
    seeds, ks = (3, 4, 5), [1, 2, 5]
    keys, out = sweep.bias_variance_vs_iterations(objects, psf_sets, seeds, ks, total_brightness=1e6)
    tasks = sweep.make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sweep.sort_by_group(tasks, objects)]
    old = sweep._bias_variance_one_sweep_per_k(tasks, keys, objects, psf_sets, ks, 1e6, 'f32', 0, None, None, 0.1)
    assert out.shape == (3, 4, 6) and np.array_equal(out, old)
    # a list the checkpoints do not take (not increasing) still runs, on the loop
    k2, out2 = sweep.bias_variance_vs_iterations(objects, psf_sets, seeds, [5, 1], total_brightness=1e6)
    assert k2 == keys and np.array_equal(out2[0], out[2]) and np.array_equal(out2[1], out[0])


def test_best_iterations_at_six_photons_per_pixel(lib, small_sweep):
    from rescan_line_sted_amd import sweep
    objects, psf_sets = small_sweep
    ks = list(range(1, 9))
    tasks, m = sweep.error_vs_iterations(objects, {'one': psf_sets['one']}, (1, 2), ks, total_brightness=6.0 * 64 * 64, dtype='f64')
    _, trace = sweep.run_tasks_checkpoints_device(tasks, objects, {'one': psf_sets['one']}, ks, total_brightness=6.0 * 64 * 64, dtype='f64',
                                                  estimates=False)
    assert np.array_equal(m['mse'], trace[..., 5] / (64 * 64))
    best = sweep.best_iterations(trace, ks)
    for t, task in enumerate(tasks):
        f5 = trace[:, t, 5]
        arg = int(np.argmin(f5))
        print('%s: field 5 over K = 1..8 %s -> best K %d' % (task, np.array2string(f5, precision=4), best[t]))
        assert best[t] == ks[arg]
        if 0 < arg < len(ks) - 1:                                       # an interior minimum: semi-convergence inside the range
            assert f5[arg] < f5[0] and f5[arg] < f5[-1]


# ------------------------------------------------------------------ error codes
def test_error_codes(lib):
    case = 'f64_two_chunks_short_last'
    _, _, ny, nx, _, _, _, _, _ = CASES[case]
    plan = make_plan(lib, case)
    objs, tb, seeds, ids = tasks_of(case)
    objs = [np.ascontiguousarray(o) for o in objs[:2]]
    T = lib.DeconvPlan._Task
    dp = ctypes.POINTER(ctypes.c_double)

    def task_array(null_object=False, image_id=0):
        a = (T * 2)()
        for i in range(2):
            a[i].object = None if (null_object and i == 1) else objs[i].ctypes.data_as(dp)
            a[i].total_brightness, a[i].seed, a[i].image_id = tb, 1, image_id
        return a
    good = task_array()
    buf = Buffer(2 * ny * nx, 'f64')
    outs = (ctypes.c_void_p * 2)(buf.address, None)

    def call(h=plan.handle, tasks=good, n=2, ks=(1, 2), n_k=None, rng=lib.RNG_PHILOX, dev_out=outs, out_dtype=lib.RL_F64):
        kl = (ctypes.c_int * max(len(ks), 1))(*ks) if ks is not None else None
        return lib.lib.rl_batch_submit_checkpoints(h, ctypes.cast(tasks, ctypes.c_void_p) if tasks is not None else None, n, kl,
                                                   len(ks) if n_k is None else n_k, rng, dev_out, out_dtype, None)
    assert call() == 0
    assert call(n=0) == 0 and call(tasks=None, n=0) == 0
    for kw in (dict(h=None), dict(tasks=None), dict(n=-1), dict(ks=None, n_k=2), dict(n_k=0), dict(n_k=-1), dict(ks=(0, 1)), dict(ks=(-1,)),
               dict(ks=(2, 2)), dict(ks=(1, 3, 2)), dict(rng=7), dict(out_dtype=5), dict(tasks=task_array(null_object=True)),
               dict(tasks=task_array(image_id=0xffffffff))):
        assert call(**kw) == RL_ERR_INVALID, kw
    assert call(out_dtype=5, dev_out=None) == 0                           # (out_dtype is not read without a destination)
    plan.ctx.synchronize()
    buf.free()
