"""Poisson draws one slice per lane ahead of the RL loops (rlsted.cpp run_slices, include/rlsted.h rl_deconv_draws_ahead;
aux_kernels.hip k_poisson: grid cap, image resolved once per tile).  Needs an MI355X.

Every case builds the same plan twice in one process, with RLSTED_DRAW_AHEAD=0 -- every slice draws at the head of its lane --
and with =1, runs the same calls on both and compares measurement and estimate with np.array_equal: the kernels and their inputs
are the same, only the stream, the moment and the width of the sampler's launch differ, so there is no tolerance.  The getter says
whether the draw stream was used: a cycle that follows nothing draws its first slice per lane in the lane, a cycle whose lanes
stayed open behind another draws every sharing slice ahead, and a lane that holds one slice, a slice that does not share and a plan
of one lane never do.  Two cases also compare the measurement with the sampler's numpy twin (oracle/philox_poisson.py).

Shapes: 128 x 128 with a 9 x 9 PSF transforms at L = 192 (general row body, which has no frame-pair kernels: the transform
length is image + half the PSF, so no PSF smaller than the image brings 128^2 to L = 256); 200 x 200 at L = 256 (wave-private
kernels, frame pairs on single-view f32 plans).  128^2 is a multiple of the sampler's 2048-pixel tile (one image per tile),
200^2 is not (tiles straddle images).  Neither PSF is rank 1, so the plans stay on the FFT path.
Slices hold two frames unless a case says otherwise: a slice shares its simulation when its classes are at most half its frames.
"""
import ctypes

import numpy as np
import pytest

from plan_cases import plans_per_value

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def psfs_of(V, side=9, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.random((1, side, side)) + 0.05 for _ in range(V)]


def objects(pattern, ny, nx, seed=11):
    rng = np.random.default_rng(seed)
    kinds = {c: rng.random((ny, nx)) * 200 + 1 for c in sorted(set(pattern))}
    return np.stack([kinds[c] for c in pattern])


def plans(lib, psfs, B, ny, nx, dtype, mb, lanes=2, switches=('0', '1'), grid=None):
    """One plan per value of RLSTED_DRAW_AHEAD.  grid: RLSTED_DRAW_GRID -- a two-frame slice of 128^2 has 16 tiles, so only a cap
    below that makes a workgroup of the background launch walk several."""
    return plans_per_value(lib, psfs, B, ny, nx, dtype, 'RLSTED_DRAW_AHEAD', switches, fft_only=True,
                           options={'RLSTED_CHUNK_MB': mb, 'RLSTED_LANES': lanes, 'RLSTED_DRAW_GRID': grid or 256})


def twin(plan, dtype, seed):
    from oracle import philox_poisson as pp
    lam = plan.noiseless()
    want = pp.noisy_measurement(lam.reshape((-1,) + lam.shape[2:]), seed).reshape(lam.shape)
    return want.astype(np.float32).astype(np.float64) if dtype == 'f32' else want


def same(off, on):
    assert np.array_equal(off.measurement(), on.measurement())
    assert np.array_equal(off.estimate(), on.estimate())


def cycles(off, on, K, reps, seed, slices, ahead):
    """The same call on both plans; `ahead`: slices of the LAST cycle the =1 plan must have drawn on the draw stream."""
    for p in (off, on):
        p.bench_cycles(K, reps, seed=seed)
    same(off, on)
    assert on.object_classes()['slices'] == slices
    assert off.draws_ahead() == 0
    assert on.draws_ahead() == ahead


# dtype, size, PSF side, V, RLSTED_CHUNK_MB for two-frame slices, frame pairs
SHAPES = {
    'f32-128': ('f32', 128, 9, 1, '0.6', False),
    'f64-128': ('f64', 128, 9, 1, '1.2', False),
    'f64-128-V2': ('f64', 128, 9, 2, '2.2', False),
    'f32-pairs-200': ('f32', 200, 9, 1, '0.001', True),
}


def shape_plans(lib, name, pattern, lanes=2, **kw):
    dtype, size, side, V, mb, pairs = SHAPES[name]
    off, on = plans(lib, psfs_of(V, side), len(pattern), size, size, dtype, mb, lanes, **kw)
    assert on.strategy()['frame_pairs'] == pairs
    for p in (off, on):
        p.set_object(objects(pattern, size, size), 3e7 * (size / 128) ** 2)
    return off, on, dtype


@pytest.mark.parametrize('name', ['f32-128', 'f32-pairs-200', 'f64-128'])
def test_two_lanes_three_slices_each(lib, name):
    """Cases 1: a lone cycle draws its first slice per lane in the lane and the other four ahead; in a cycle behind another all
    six.  The last cycle's measurement is the numpy twin's."""
    off, on, dtype = shape_plans(lib, name, 'AABBAAAABBAA')
    cycles(off, on, 3, 1, 5, slices=6, ahead=4)
    cycles(off, on, 3, 2, (1 << 40) + 3, slices=6, ahead=6)
    assert on.object_classes()['shared_slices'] == 6 and on.simulated_images() == 2
    assert np.array_equal(on.measurement(), twin(on, dtype, (1 << 40) + 3 + 1))   # (cycle r of a call draws with seed + r)


@pytest.mark.parametrize('frames,slices,lone,chained', [(14, 7, 4, 7), (8, 4, 1, 2)])
def test_three_lanes_and_a_slice_count_that_is_no_multiple(lib, frames, slices, lone, chained):
    """Case 2.  Seven slices: lanes of 3, 2 and 2.  Four slices: lanes 1 and 2 hold ONE slice each -- its draw in a chained cycle
    would overwrite the measurement that very slice of the cycle before still iterates on, so they keep the in-lane draw while
    lane 0 draws both of its slices ahead."""
    off, on, _ = shape_plans(lib, 'f64-128', ('AABB' * 4)[:frames], lanes=3)
    cycles(off, on, 2, 1, 5, slices=slices, ahead=lone)
    cycles(off, on, 2, 3, 6, slices=slices, ahead=chained)


def test_one_slice_per_lane_falls_back(lib):
    """Case 3: the slice a draw would run beside is the slice whose measurement it writes."""
    off, on, _ = shape_plans(lib, 'f64-128', 'AABB')
    cycles(off, on, 2, 1, 5, slices=2, ahead=0)
    cycles(off, on, 2, 3, 6, slices=2, ahead=0)


def test_one_lane_has_no_draw_stream(lib):
    """Case 4."""
    off, on, _ = shape_plans(lib, 'f64-128', 'AABBAAAABBAA', lanes=1)
    cycles(off, on, 2, 2, 5, slices=6, ahead=0)


def test_sharing_and_per_frame_slices_alternate(lib):
    """Case 5: slices of four frames, A A A A | A B C D | A A A A | B B B B | A B C D | A A A A.  Slices 1 and 4 hold four classes
    in four frames: they simulate every frame in their lane's spectrum space and draw there."""
    pattern = 'AAAAABCDAAAABBBBABCDAAAA'
    off, on = plans(lib, psfs_of(1), len(pattern), 128, 128, 'f64', '2.0')
    for p in (off, on):
        p.set_object(objects(pattern, 128, 128), 3e7)
    cycles(off, on, 2, 1, 5, slices=6, ahead=3)     # slices 2, 3 and 5
    cycles(off, on, 2, 2, 6, slices=6, ahead=4)     # and slice 0
    assert on.object_classes()['shared_slices'] == 4
    assert np.array_equal(off.noiseless(), on.noiseless())


def test_two_views(lib):
    """Case 6."""
    off, on, _ = shape_plans(lib, 'f64-128-V2', 'AABBAAAABBAA', grid=5)
    cycles(off, on, 2, 1, 5, slices=6, ahead=4)
    cycles(off, on, 2, 2, 6, slices=6, ahead=6)


def test_tiles_that_straddle_images(lib):
    """Case 7: 200^2 = 40000 pixels is no multiple of the 2048-pixel tile -- the sampler's per-pixel image lookup."""
    off, on, dtype = shape_plans(lib, 'f32-pairs-200', 'AABBAAAABBAA', grid=7)
    cycles(off, on, 2, 1, 5, slices=6, ahead=4)
    cycles(off, on, 2, 2, 77, slices=6, ahead=6)
    assert np.array_equal(on.measurement(), twin(on, dtype, 78))


@pytest.mark.parametrize('K', [1, 20])
def test_chained_cycles(lib, K):
    """Case 8: four cycles whose lanes never meet.  K = 1: a draw is long against the loop it runs beside, so the draw stream
    runs into its throttle, and every cycle's draws overwrite the measurements of the cycle before."""
    off, on, dtype = shape_plans(lib, 'f32-pairs-200', 'AABBAAAABBAA', grid=3)
    cycles(off, on, K, 4, 900, slices=6, ahead=6)
    assert np.array_equal(on.measurement(), twin(on, dtype, 903))
    cycles(off, on, K, 4, 17, slices=6, ahead=6)


def test_a_new_object_with_another_class_layout(lib):
    """Case 9: the compact buffers are rebuilt for the second object after the first cycle's draws; a plan that only ever saw
    the second object computes the same."""
    first, second = 'AABBAAAABBAA', 'CCCCCCDDEEEE'
    dtype, size, side, V, mb, _ = SHAPES['f32-pairs-200']
    off, on, fresh = plans(lib, psfs_of(V, side), 12, size, size, dtype, mb, switches=('0', '1', '1'))
    for p in (off, on):
        p.set_object(objects(first, size, size), 3e7)
    cycles(off, on, 2, 2, 5, slices=6, ahead=6)
    for p in (off, on, fresh):
        p.set_object(objects(second, size, size, seed=41), 5e7)
    fresh.bench_cycles(2, 1, seed=6)
    cycles(off, on, 2, 1, 6, slices=6, ahead=4)
    same(fresh, on)
    assert on.object_classes() == {'classes': 3, 'shared_slices': 6, 'slices': 6}


def test_batch_run_with_per_frame_keys(lib):
    """Case 10: rl_batch_run over two chunks of six two-frame slices; every task has its own seed and image id."""
    from oracle import philox_poisson as pp
    dtype, size, side, V, mb, _ = SHAPES['f64-128-V2']
    B, n_tasks, K = 12, 20, 2
    off, on = plans(lib, psfs_of(V, side), B, size, size, dtype, mb)
    kinds = objects('ABC', size, size)
    which = [0, 0, 1, 1, 0, 0, 2, 2, 0, 0, 1, 1] + [2, 2, 0, 0, 0, 0, 1, 1]
    tasks = (lib.DeconvPlan._Task * n_tasks)()
    for i, w in enumerate(which):
        tasks[i].object = kinds[w].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        tasks[i].total_brightness = 3e7
        tasks[i].seed = 1000 + 7 * i
        tasks[i].image_id = 50 - i
    got = []
    for p in (off, on):
        out = np.empty((n_tasks, size, size))
        lib.check(lib.lib.rl_batch_run(p.handle, ctypes.cast(tasks, ctypes.c_void_p), n_tasks, K, lib.RNG_PHILOX, lib.ptr(out)))
        got.append((out, p.measurement(), p.noiseless()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    # the last chunk: tasks 12 .. 19 and the last one four times more -- six sharing slices, a chunk follows nothing
    assert on.object_classes()['shared_slices'] == 6 and on.object_classes()['slices'] == 6
    assert off.draws_ahead() == 0 and on.draws_ahead() == 4
    meas, lam = got[1][1], got[1][2]
    for f, t in enumerate(list(range(12, 20)) + [19] * 4):
        for v in range(V):
            want = pp.poisson(lam[f, v].ravel(), 1000 + 7 * t, (50 - t) * V + v).reshape(size, size) + 1e-9
            assert np.array_equal(meas[f, v], want), (f, v)


@pytest.mark.parametrize('K', [0, 2])
def test_timing_a_cycle_that_draws_ahead(lib, K):
    """Case 11: rl_deconv_time_cycle runs the draws as production does -- the sampler's events bracket its launch on the draw
    stream -- and counts what test_gpu_class_poisson.py::test_timing_a_cycle_counts_the_class_simulation counts."""
    off, on = plans(lib, psfs_of(1), 24, 128, 128, 'f64', '2.0')
    res = []
    for p in (off, on):
        p.set_object(objects('A' * 24, 128, 128), 3e7)
        avg = (ctypes.c_double * 8)()
        launches = (ctypes.c_double * 8)()
        fpl = ctypes.c_double()
        lib.check(lib.lib.rl_deconv_time_cycle(p.handle, K, lib.RNG_PHILOX, ctypes.c_uint64(3), avg, launches, ctypes.byref(fpl)))
        res.append((list(avg), list(launches)))
    same(off, on)
    info = on.object_classes()
    assert info['slices'] == 6 and info['shared_slices'] == 6 and on.simulated_images() == 1
    assert off.draws_ahead() == 0 and on.draws_ahead() == 4
    (avg, launches), (_, launches_off) = res[1], res[0]
    assert launches == launches_off
    assert launches[5] == 1 and launches[6] == 6      # one class simulation (its ROW_INV), the sampler once per slice
    if K == 0:   # its column pass; its ROW_FWD beside the one K = 0 runs per slice for the estimate's spectrum
        assert launches[0] == 1 and launches[4] == 1 + 6 and launches[1] == 0 and launches[3] == 0
    assert all(np.isfinite(a) for a in avg) and avg[6] > 0.0
